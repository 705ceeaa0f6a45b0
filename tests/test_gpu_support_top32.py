"""The head of an fp32 support order by the selection kernel (jstsp_support_top_c32, csrc/support_top.hip; support_top): bit
equality with support_order(S)[:, :count] and with the stable host argsort of the fp32 key (tests/drift_ref.py, the reference of
tests/test_gpu_support_order.py) at g = 12, 1000, 1025, 8192 and 32768 - below one workgroup's stride, either side of it, the
solver's shapes - and count = 1, 40, g (g <= 4096) and 4096.  Each size runs a batch of three trials: a continuous one whose
neighbouring fp32 keys are more than 4 ulp apart (no contraction of x*x + y*y can reorder it against the host), one drawn from
TIE_VALUES with NaN entries (|1e-30|^2 underflows in fp32: it ties with zero), and one whose non-zero part has min(g, 4096) - 1
entries, so that at count = min(g, 4096) the strict part holds count - 1 entries (4095 at the two large sizes) and the last
place goes to the first of a zero tie class.  In the TIE_VALUES trial every class holds about g / 7 entries, so from g = 1000 on
the threshold of count 1 and 40 lies inside a class larger than count; an all-zero trial is one class, zero's.  A trial's list
depends on neither its batch mates nor the memspace.  The rank output is covered through the solver
(tests/test_gpu_refresh32.py); directly: S of a one-iteration refreshed call is zero off the list.  The refusals."""
import functools

import numpy as np
import pytest
import torch

import drift_ref as D
import jstsp19_amd as J
from test_drift_ref import TIE_VALUES, continuous_trial, keys_are_separated

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
SHAPES = {12: (3, 4), 1000: (25, 40), 1025: (25, 41), 8192: (64, 128), 32768: (64, 512)}
TOP_MAX = 4096


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).cuda())


@functools.lru_cache(maxsize=None)
def _trials(g):
    """(S complex64 (3, Gr, G2), the host order int32 (3, g))"""
    shape = SHAPES[g]
    rng = np.random.default_rng(g)
    cont = continuous_trial(seed=29, shape=shape).astype(np.complex64)
    assert keys_are_separated(cont, np.float32)
    ties = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=shape)].astype(np.complex64)
    for k in rng.choice(g, 3, replace=False):
        ties[np.unravel_index(k, shape, order="F")] = complex(np.nan, 1.0) if k % 2 else complex(-np.nan, np.nan)
    # a zero tie class in the front part as well, and a strict part of min(g, 4096) - 1 entries
    sparse = continuous_trial(seed=31, shape=shape).astype(np.complex64).reshape(-1, order="F")
    assert keys_are_separated(sparse, np.float32)
    keep = rng.choice(g, min(g, TOP_MAX) - 1, replace=False)
    flat = np.zeros(g, np.complex64)
    flat[keep] = sparse[keep]
    S = np.stack([cont, ties, flat.reshape(shape, order="F")])
    want = np.stack([D.support_order_ref(s, np.float32) for s in S])
    return S, want


def _counts(g):
    return sorted({c for c in (1, 40, g if g <= TOP_MAX else TOP_MAX) if c <= min(g, TOP_MAX)})


@pytest.mark.parametrize("g", sorted(SHAPES))
def test_the_head_of_the_order_on_the_bits(g):
    S, want = _trials(g)
    dS = _dev(S)
    full = J.support_order(dS).cpu().numpy()
    np.testing.assert_array_equal(full, want)                   # the device's own full order is the host's
    top = min(g, TOP_MAX)
    # the third trial: count - 1 strict entries at the largest count, then the first zero by index
    assert np.count_nonzero(S[2]) == top - 1
    for count in _counts(g):
        got = J.support_top(dS, count)
        assert got.dtype == torch.int32 and tuple(got.shape) == (3, count)
        np.testing.assert_array_equal(got.cpu().numpy(), want[:, :count], err_msg="g %d count %d" % (g, count))
        np.testing.assert_array_equal(got.cpu().numpy(), full[:, :count])
        for t in range(3):                                      # a trial alone: no dependence on its batch mates
            assert torch.equal(J.support_top(J.colmajor(dS[t:t + 1]), count)[0], got[t]), (g, count, t)
        host = J.support_top(S, count)                          # the host memspace: the same bits
        assert isinstance(host, np.ndarray) and host.dtype == np.int32
        np.testing.assert_array_equal(host, got.cpu().numpy())


def test_nan_first_and_a_zero_class_larger_than_count():
    S, want = _trials(1000)
    k = D.support_key(S[1], np.float32)
    assert np.isnan(k[want[1, :3] - 1]).all() and not np.isnan(k[want[1, 3] - 1])      # the NaNs lead, in index order
    assert list(want[1, :3]) == sorted(want[1, :3])
    zeros = np.flatnonzero(D.support_key(S[1], np.float32) == 0)
    assert zeros.size > 40                                      # 0 and 1e-30 tie in fp32: a class larger than count = 40
    Z = np.zeros((2, 64, 128), np.complex64)                    # an all-zero trial: the class is the trial
    for count in (1, 40, 4096):
        np.testing.assert_array_equal(J.support_top(_dev(Z), count).cpu().numpy(), np.tile(np.arange(1, count + 1, dtype=np.int32), (2, 1)))


def test_the_rank_through_the_solver_s_is_zero_off_the_list():
    import refresh32_problems as Q
    p = Q.problem("R1")
    S, _, _, st, order = J.proposed_algorithm_refresh(p["subY"], p["Omega"], p["A"], p["B"], 1, p["tau_Y"], p["tau_S"], p["rho"], start=0, period=0)
    N, M, Gr, G2 = Q.SHAPES["R1"]
    g = Gr * G2
    v = st[:, 4 * N * M:4 * N * M + g].reshape(Q.BATCH, G2, Gr).transpose(0, 2, 1)
    np.testing.assert_array_equal(order, J.support_top(np.ascontiguousarray(v), g))
    flat = S.transpose(0, 2, 1).reshape(Q.BATCH, g)
    for t in range(Q.BATCH):
        off = np.setdiff1d(np.arange(g), order[t, :15] - 1)
        assert not flat[t, off].any() and flat[t].any()


def test_refusals_leave_the_output_untouched():
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    fn = ctx._lib.jstsp_support_top_c32
    last = lambda: _lib.load().jstsp_last_error().decode()
    S = torch.zeros(2 * 2 * 12, dtype=torch.float32, device="cuda")
    ix = torch.full((24,), -7, dtype=torch.int32, device="cuda")
    hS, hix = np.zeros(2 * 2 * 12, np.float32), np.full(24, -7, dtype=np.int32)
    for ms, s, o in ((_lib.DEVICE, S.data_ptr(), ix.data_ptr()), (_lib.HOST, hS.ctypes.data, hix.ctypes.data)):
        for dims in ((0, 4, 2), (3, -1, 2), (3, 4, 0), (65536, 32768, 1)):
            assert fn(ctx.handle, *dims, s, 1, o, ms) == E_SHAPE, dims
            assert last().startswith("support_top: ")
        assert fn(ctx.handle, 3, 4, 2, None, 3, o, ms) == E_NULL
        assert fn(ctx.handle, 3, 4, 2, s, 3, None, ms) == E_NULL
        for count in (0, 13):                                   # count = 0 and count = g + 1
            assert fn(ctx.handle, 3, 4, 2, s, count, o, ms) == E_ARG, count
            assert last().startswith("support_top: count = %d" % count)
        assert fn(ctx.handle, 3, 4, 2, s, 3, o, 7) == E_ARG     # a bad memspace
        torch.cuda.synchronize()
        assert bool((ix == -7).all()) if ms == _lib.DEVICE else np.all(hix == -7)
        assert fn(ctx.handle, 3, 4, 2, s, 12, o, ms) == 0       # and the context then selects: all zero gives 1..12 per trial
        torch.cuda.synchronize()
    want = np.tile(np.arange(1, 13, dtype=np.int32), 2)
    np.testing.assert_array_equal(ix.cpu().numpy(), want)
    np.testing.assert_array_equal(hix, want)
    big = torch.zeros(2 * 64 * 128, dtype=torch.float32, device="cuda")     # above 4096 entries the limit is the list's
    out = torch.full((4097,), -7, dtype=torch.int32, device="cuda")
    assert fn(ctx.handle, 64, 128, 1, big.data_ptr(), 4097, out.data_ptr(), _lib.DEVICE) == E_ARG
    assert fn(ctx.handle, 64, 128, 1, big.data_ptr(), 4096, out.data_ptr(), _lib.DEVICE) == 0
    torch.cuda.synchronize()
    assert int(out[4095]) == 4096 and int(out[4096]) == -7
