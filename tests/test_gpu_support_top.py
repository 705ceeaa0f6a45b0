"""The head of a support order by the selection kernel (jstsp_support_top_f64, csrc/support_top.hip; support_top_f64): exact
against support_order_f64(V)[:, :count] and against the stable host argsort of tests/drift_ref.py - duplicate magnitudes across
the threshold, a NaN and an +Inf, the smallest sizes and sizes either side of a wave multiple, count = 1 and count = g, a tie class
larger than the kernel's LDS list, the largest count, values near both ends of the exponent range, an all-zero trial - independent
of batch and memspace, and the refusals.  The continuous trials keep neighbouring keys more than 4 ulp apart (keys_are_separated):
no contraction of x*x + y*y can reorder them against the host."""
import numpy as np
import pytest
import torch

import drift_ref as D
import jstsp19_amd as J
from test_drift_ref import TIE_VALUES, continuous_trial, keys_are_separated

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ARG = -1, -2, -4


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).cuda())


def _ref(S):
    S = np.asarray(S)
    return np.stack([D.support_order_ref(s, np.float64) for s in (S if S.ndim == 3 else S[None])])


def _check(S, counts, memspaces=("device",)):
    """support_top_f64 of S (batch, Gr, G2) at every count against the host order and the device's own full order."""
    want = _ref(S)
    dS = _dev(S)
    full = J.support_order_f64(dS).cpu().numpy()
    np.testing.assert_array_equal(full, want)
    for count in counts:
        for ms in memspaces:
            got = J.support_top_f64(dS if ms == "device" else S, count)
            assert got.dtype == (torch.int32 if ms == "device" else np.int32) and tuple(got.shape) == (S.shape[0], count)
            got = got.cpu().numpy() if ms == "device" else got
            np.testing.assert_array_equal(got, want[:, :count], err_msg="count %d, %s" % (count, ms))


def engineered():
    """6 x 4 x 3: every trial draws from values whose keys tie exactly (|3+4j|^2 == |5|^2, |1|^2 == |1j|^2 == |-1|^2, zeros), so at
    most counts the threshold falls inside a tie class; the last trial also holds a NaN and an +Inf."""
    rng = np.random.default_rng(5)
    t = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=(3, 6, 4))]
    t[2, 1, 2] = complex(np.nan, 1.0)
    t[2, 3, 0] = complex(2.0, -np.inf)
    t[2, 5, 3] = complex(-np.nan, np.nan)
    return t


def test_engineered_ties_across_the_threshold_a_nan_and_an_inf():
    S = engineered()
    want = _ref(S)
    assert list(want[2, :3]) == [14, 24, 4]                     # the NaNs in index order, then the Inf
    _check(S, range(1, 25), ("device", "host"))
    one = J.support_top_f64(_dev(S[2]), 5)                      # (Gr, G2) in: one trial
    assert tuple(one.shape) == (1, 5)
    np.testing.assert_array_equal(one.cpu().numpy(), want[2:3, :5])


@pytest.mark.parametrize("shape", [(1, 1), (15, 17), (257, 1)], ids=["g1", "g255", "g257"])
def test_small_sizes_count_1_and_count_g(shape):
    g = shape[0] * shape[1]
    cont = continuous_trial(seed=11, shape=shape)
    assert keys_are_separated(cont, np.float64)
    rng = np.random.default_rng(g)
    ties = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=shape)]
    S = np.stack([cont, ties])
    _check(S, sorted({1, min(2, g), (g + 1) // 2, max(g - 1, 1), g}), ("device", "host"))


def test_a_tie_class_larger_than_the_lds_list():
    """64 x 128 with 6000 exact zeros: 2192 entries precede them, so the 4096-th key is zero's and 1904 of the 6000 are admitted."""
    S = continuous_trial(seed=13, shape=(64, 128))
    assert keys_are_separated(S, np.float64)
    flat = S.reshape(-1, order="F").copy()
    zeros = np.sort(np.random.default_rng(17).choice(flat.size, 6000, replace=False))
    flat[zeros] = 0
    S = flat.reshape(64, 128, order="F")[None]
    want = _ref(S)
    np.testing.assert_array_equal(want[0, 2192:4096], zeros[:1904] + 1)
    _check(S, (4096, 2192, 2193, 1))


def test_a_64_x_512_trial_at_the_largest_count_and_at_the_solvers_last():
    S = continuous_trial()
    assert S.shape == (64, 512) and keys_are_separated(S, np.float64)
    _check(S[None], (4096, 510, 110))


@pytest.mark.parametrize("exp", [500, -500])
def test_values_scaled_to_either_end_of_the_exponent_range(exp):
    S = continuous_trial(seed=19, shape=(32, 16)) * 2.0 ** exp  # keys near 2^+-1000: every byte of the key takes part
    S[3, 4] = 0
    assert np.all(np.isfinite(D.support_key(S, np.float64))) and np.count_nonzero(D.support_key(S, np.float64)) == 511
    _check(S[None], (1, 35, 511, 512))
    np.testing.assert_array_equal(_ref(S[None]), _ref(S[None] * 2.0 ** -exp))


def test_an_all_zero_trial():
    for shape, count in (((5, 7), 35), ((5, 7), 4), ((64, 128), 4096)):
        got = J.support_top_f64(_dev(np.zeros((2,) + shape, complex)), count).cpu().numpy()
        np.testing.assert_array_equal(got, np.tile(np.arange(1, count + 1, dtype=np.int32), (2, 1)))


def test_a_list_does_not_depend_on_batch_or_memspace():
    rng = np.random.default_rng(23)
    S = np.stack([continuous_trial(seed=s, shape=(24, 20)) for s in range(4)] + [TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=(24, 20))]])
    dS = _dev(S)
    for count in (1, 37, 480):
        full = J.support_top_f64(dS, count)
        for t in range(5):
            assert torch.equal(J.support_top_f64(J.colmajor(dS[t:t + 1]), count)[0], full[t])
        host = J.support_top_f64(S, count)
        assert isinstance(host, np.ndarray) and host.dtype == np.int32
        np.testing.assert_array_equal(host, full.cpu().numpy())


def test_refusals_leave_the_output_untouched():
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    fn = ctx._lib.jstsp_support_top_f64
    last = lambda: _lib.load().jstsp_last_error().decode()
    S = torch.zeros(2 * 2 * 12, dtype=torch.float64, device="cuda")
    ix = torch.full((24,), -7, dtype=torch.int32, device="cuda")
    hS, hix = np.zeros(2 * 2 * 12), np.full(24, -7, dtype=np.int32)
    for ms, s, o in ((_lib.DEVICE, S.data_ptr(), ix.data_ptr()), (_lib.HOST, hS.ctypes.data, hix.ctypes.data)):
        for dims in ((0, 4, 2), (3, -1, 2), (3, 4, 0), (65536, 32768, 1)):
            assert fn(ctx.handle, *dims, s, 1, o, ms) == E_SHAPE, dims
            assert "support_top" in last()
        assert fn(ctx.handle, 3, 4, 2, None, 3, o, ms) == E_NULL
        assert fn(ctx.handle, 3, 4, 2, s, 3, None, ms) == E_NULL
        for count in (0, -1, 13, 4097):
            assert fn(ctx.handle, 3, 4, 2, s, count, o, ms) == E_ARG, count
            assert "count" in last()
        assert fn(ctx.handle, 3, 4, 2, s, 3, o, 7) == E_ARG     # a bad memspace
        torch.cuda.synchronize()
        assert bool((ix == -7).all()) if ms == _lib.DEVICE else np.all(hix == -7)    # (the other one is filled by its own turn)
        assert fn(ctx.handle, 3, 4, 2, s, 12, o, ms) == 0       # and the context then selects: all zero gives 1..12 per trial
        torch.cuda.synchronize()
    want = np.tile(np.arange(1, 13, dtype=np.int32), 2)
    np.testing.assert_array_equal(ix.cpu().numpy(), want)
    np.testing.assert_array_equal(hix, want)
    # above 4096 entries the limit is the list's, not the trial's
    big = torch.zeros(2 * 64 * 128, dtype=torch.float64, device="cuda")
    out = torch.full((4097,), -7, dtype=torch.int32, device="cuda")
    assert fn(ctx.handle, 64, 128, 1, big.data_ptr(), 4097, out.data_ptr(), _lib.DEVICE) == E_ARG
    assert fn(ctx.handle, 64, 128, 1, big.data_ptr(), 4096, out.data_ptr(), _lib.DEVICE) == 0
    torch.cuda.synchronize()
    assert int(out[4095]) == 4096 and int(out[4096]) == -7
