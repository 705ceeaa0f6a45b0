"""The order of a support widened over neighbouring angle cells (jstsp_support_order_wide_c32 / _f64, csrc/support.hip;
support_order_wide, support_order_wide_f64): exact against the numpy reference of tests/wide_ref.py on engineered trials, sizes
that are no multiple of anything, a full-size trial, delay blocks larger than the kernel's LDS tile (the halo path) and a radius
above what one launch takes; radius 0 against support_order*; independent of batch and memspace; usable as the indx_S of
proposed_algorithm_angles_f64; and the refusals."""
import numpy as np
import pytest
import torch

import wide_ref as W
import jstsp19_amd as J
from test_drift_ref import continuous_trial, keys_are_separated, tie_trials
from test_gpu_tracking import SMALL, _sp

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ARG = -1, -2, -4
SOW_TILE = 64           # csrc/support.hip: the LDS tile is at most SOW_TILE x SOW_TILE keys, halo included
SOW_HALO = 8            # csrc/support.hip: the largest radius one launch takes on a tiled axis
FORMS = [pytest.param(J.support_order_wide, np.complex64, np.float32, id="c32"),
         pytest.param(J.support_order_wide_f64, np.complex128, np.float64, id="f64")]
GR, GT, NL = 6, 4, 3
RADII = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 1)]


def _dev(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).cuda())


def _ref(S, Gt, wr, wt, primary, real):
    S = np.asarray(S)
    return np.stack([W.support_order_wide_ref(s, Gt, wr, wt, primary, real) for s in (S if S.ndim == 3 else S[None])])


def engineered_trials():
    """Five 6 x (4*3) trials of small integers, whose keys are exact in both precisions."""
    rng = np.random.default_rng(5)
    corners = np.zeros((GR, GT * NL), complex)                  # spikes in all four corners of block 1, and one in block 2
    for v, (r, g) in enumerate(((0, 0), (GR - 1, 0), (0, GT - 1), (GR - 1, GT - 1))):
        corners[r, GT + g] = 2 + v
    corners[2, 2 * GT + 1] = 1j
    overlap = np.zeros((GR, GT * NL), complex)                  # two spikes whose windows overlap, the weaker one first in index
    overlap[2, 1], overlap[3, 2] = 3, 4 + 3j
    overlap[4, 2 * GT] = 3                                      # and an equal of the first in another block
    values = np.array([0, 1, 1j, -1, 3 + 4j, 5, 2], dtype=complex)
    equal = values[rng.integers(0, values.size, size=(GR, GT * NL))]
    zero = np.zeros((GR, GT * NL), complex)
    odd = values[rng.integers(0, values.size, size=(GR, GT * NL))]
    odd[1, 2] = complex(np.nan, 1.0)
    odd[GR - 1, GT * NL - 1] = complex(2.0, -np.inf)
    return np.stack([corners, overlap, equal, zero, odd])


# ---- 1. exact against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_engineered_trials(order, cdtype, real, primary):
    trials = engineered_trials().astype(cdtype)
    dev = _dev(trials)
    for wr, wt in RADII:
        want = _ref(trials, GT, wr, wt, primary, real)
        np.testing.assert_array_equal(want[3], np.arange(1, GR * GT * NL + 1))       # all zero: 1..72
        for sel in (slice(0, 1), slice(1, 4), slice(None)):     # batch 1, 3 and all
            got = order(J.colmajor(dev[sel]), GT, wr, wt, primary=primary)
            assert got.dtype == torch.int32 and got.is_cuda
            np.testing.assert_array_equal(got.cpu().numpy(), want[sel], err_msg="device, radius %r" % ((wr, wt),))
            host = order(trials[sel], GT, wr, wt, primary=primary)                   # numpy in: the host memspace
            assert isinstance(host, np.ndarray) and host.dtype == np.int32
            np.testing.assert_array_equal(host, want[sel], err_msg="host, radius %r" % ((wr, wt),))
    one = order(_dev(trials[4]), GT, primary=primary)           # (Gr, G2) in: one trial, the default radius (1, 1)
    assert one.shape == (1, GR * GT * NL)
    np.testing.assert_array_equal(one.cpu().numpy(), _ref(trials[4], GT, 1, 1, primary, real))


@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_sizes_that_are_no_multiple_of_anything(order, cdtype, real, primary):
    trials = tie_trials().astype(cdtype)                        # (5, 5, 7) as Gr = 5, Gt = 7, L = 1
    for wr, wt in ((2, 3), (1, 2)):                             # (2, 3): the largest legal window, the whole block
        np.testing.assert_array_equal(order(_dev(trials), 7, wr, wt, primary=primary).cpu().numpy(),
                                      _ref(trials, 7, wr, wt, primary, real))


@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_a_64_x_512_trial(order, cdtype, real, primary):
    S = continuous_trial().astype(cdtype)                       # Gt = 64, L = 8: every delay block is one whole LDS tile
    assert S.shape == (SOW_TILE, 8 * SOW_TILE) and keys_are_separated(S, real)
    dev = _dev(S)
    for wr, wt in ((1, 1), (2, 3)):
        np.testing.assert_array_equal(order(dev, 64, wr, wt, primary=primary).cpu().numpy(), _ref(S, 64, wr, wt, primary, real))


def sparse_integers(Gr, G2, seed):
    """Zeros and about 3 % small Gaussian integers: exact keys in both precisions, most of them equal."""
    rng = np.random.default_rng(seed)
    S = np.zeros((Gr, G2), complex)
    hit = rng.random((Gr, G2)) < 0.03
    S[hit] = rng.integers(-4, 5, size=hit.sum()) + 1j * rng.integers(-4, 5, size=hit.sum())
    return S


@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_the_halo_path_of_a_block_wider_than_the_tile(order, cdtype, real, primary):
    """Gr = 64, Gt = 512, L = 1: the rows are one ring inside the tile, the 512 transmit cells are tiled with SOW_TILE - 2 wt
    interior columns and a halo that is read through the ring.  Spikes on rows 0 and 63 of the first and last column of every
    tile, for each radius used."""
    Gr, Gt = SOW_TILE, 8 * SOW_TILE
    S = sparse_integers(Gr, Gt, 21)
    for wt in (1, 3):
        n = SOW_TILE - 2 * wt                                   # interior columns of a tile
        for c0 in range(0, Gt, n):
            for c in (c0, min(c0 + n, Gt) - 1):
                S[0, c] = 5 + (c % 7)
                S[Gr - 1, c] = 6 + (c % 5) * 1j
    S = S.astype(cdtype)
    dev = _dev(S)
    for wr, wt in ((1, 1), (2, 3), (0, 1)):
        np.testing.assert_array_equal(order(dev, Gt, wr, wt, primary=primary).cpu().numpy(), _ref(S, Gt, wr, wt, primary, real),
                                      err_msg="radius %r" % ((wr, wt),))


@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("order,cdtype,real", FORMS)
def test_both_axes_tiled_and_a_radius_above_one_launch(order, cdtype, real, primary):
    """150 x 70 x 2: both axes exceed SOW_TILE, neither is a multiple of a tile's interior, and the radii (10, 9) exceed SOW_HALO,
    so the window is the composition of two launches."""
    Gr, Gt, L = 2 * SOW_TILE + 22, SOW_TILE + 6, 2
    S = sparse_integers(Gr, Gt * L, 22)
    for r in (0, 47, 48, 61, 62, Gr - 1):                       # tile edges at interiors 48 (radius 8) and 62 (radius 1), and the ring's
        for c in (0, 47, 48, 61, 62, Gt - 1, Gt, Gt * L - 1):
            S[r, c] = 1 + (r + c) % 6
    S = np.stack([S, np.roll(S, (3, 5), axis=(0, 1))]).astype(cdtype)
    dev = _dev(S)
    for wr, wt in ((SOW_HALO + 2, SOW_HALO + 1), (1, 1), (SOW_HALO, 0)):
        np.testing.assert_array_equal(order(dev, Gt, wr, wt, primary=primary).cpu().numpy(), _ref(S, Gt, wr, wt, primary, real),
                                      err_msg="radius %r" % ((wr, wt),))


# ---- 2. radius 0, batch, memspace, the solver --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("primary", W.PRIMARIES)
@pytest.mark.parametrize("kw,batch", [(SMALL, 4), (dict(Nt=64, Nr=64, L=8, T=2, Mr=8), 3)], ids=["small", "configs1_order"])
def test_radius_0_is_support_order_and_the_builders_indx_s(kw, batch, primary):
    from jstsp19_amd.system_model import build_trials
    p = _sp(**kw)
    out = build_trials(p, 1, batch, seed=9)
    got = J.support_order_wide(out["Zbar"], p.Gt, 0, 0, primary=primary)
    assert torch.equal(got, out["indx_S"]) and torch.equal(got, J.support_order(out["Zbar"]))
    zb = J.colmajor(out["Zbar"].to(torch.complex128))
    assert torch.equal(J.support_order_wide_f64(zb, p.Gt, 0, 0, primary=primary), J.support_order_f64(zb))


@pytest.fixture(scope="module")
def solved():
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=4, Nr=32, L=4, T=5, Mr=4)
    inp = build_trials(p, 0, 3, seed=4)
    assert p.solver_shape[2:] == (32, 16) and p.Gt == 4
    args = (inp["subY"], inp["Omega"], inp["A"], inp["B"], 5, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    Sm = J.proposed_algorithm_f64(*args, indx_S=inp["indx_S"], want_ce=False)[0]       # masked and thresholded: mostly exact zeros
    torch.cuda.synchronize()
    return p, inp, Sm


@pytest.mark.parametrize("primary", W.PRIMARIES)
def test_an_order_does_not_depend_on_batch_or_memspace(solved, primary):
    p, inp, Sm = solved
    for order, x, real in ((J.support_order_wide_f64, Sm, np.float64), (J.support_order_wide, J.colmajor(inp["Zbar"]), np.float32)):
        full = order(x, 4, 2, 1, primary=primary)
        np.testing.assert_array_equal(full.cpu().numpy(), _ref(x.cpu().numpy(), 4, 2, 1, primary, real))
        for t in range(3):
            assert torch.equal(order(J.colmajor(x[t:t + 1]), 4, 2, 1, primary=primary)[0], full[t])
        assert torch.equal(order(J.colmajor(x[1:3]), 4, 2, 1, primary=primary), full[1:3])
        np.testing.assert_array_equal(order(x.cpu().numpy(), 4, 2, 1, primary=primary), full.cpu().numpy())


def test_round_trip_through_proposed_algorithm_angles(solved):
    p, inp, _ = solved
    zb = J.colmajor(inp["Zbar"].to(torch.complex128))
    args = (inp["subY"], inp["Omega"])
    rest = (inp["A"], inp["B"], 5, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    a = J.proposed_algorithm_angles_f64(*args, J.support_order_wide_f64(zb, 4, 0, 0), *rest, want_ce=False)
    b = J.proposed_algorithm_angles_f64(*args, inp["indx_S"], *rest, want_ce=False)
    c = J.proposed_algorithm_angles_f64(*args, J.support_order_wide_f64(zb, 4, 1, 1), *rest, want_ce=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(c[0], b[0])                          # the widened order reaches the solver: the mask binds at Imax 5


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,size", [("jstsp_support_order_wide_c32", 8), ("jstsp_support_order_wide_f64", 16)])
def test_refusals_leave_the_output_untouched(entry, size):
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    fn = getattr(ctx._lib, entry)
    n = GR * GT * NL
    S = torch.zeros(2 * n * size // 8, dtype=torch.float64, device="cuda")
    ix = torch.full((2 * n,), -7, dtype=torch.int32, device="cuda")
    hS, hix = np.zeros(2 * n * size // 8), np.full(2 * n, -7, dtype=np.int32)
    shape = (GR, GT, NL, 2)
    refused = [((0, GT, NL, 2), (1, 1, 0), E_SHAPE), ((GR, -1, NL, 2), (1, 1, 0), E_SHAPE), ((GR, GT, 0, 2), (1, 1, 0), E_SHAPE),
               ((GR, GT, NL, 0), (1, 1, 0), E_SHAPE),
               ((64, 32769, 1, 1), (1, 1, 0), E_SHAPE),         # Gr*Gt*L = 2^21 + Gr
               ((64, 4096, 9, 1), (0, 0, 1), E_SHAPE),          # 2^21 + 2^18, at radius 0 too
               (shape, (-1, 1, 0), E_ARG), (shape, (1, -1, 1), E_ARG),
               (shape, (3, 1, 0), E_ARG),                       # 2*wr+1 = 7 > Gr = 6
               (shape, (1, 2, 0), E_ARG),                       # 2*wt+1 = 5 > Gt = 4
               (shape, (1, 1, 2), E_ARG), (shape, (0, 0, -1), E_ARG)]
    for ms, s, o in ((_lib.DEVICE, S.data_ptr(), ix.data_ptr()), (_lib.HOST, hS.ctypes.data, hix.ctypes.data)):
        for dims, (wr, wt, primary), code in refused:
            assert fn(ctx.handle, *dims, s, wr, wt, primary, o, ms) == code, (dims, wr, wt, primary)
            assert "support_order_wide" in _lib.load().jstsp_last_error().decode()
        assert fn(ctx.handle, *shape, None, 1, 1, 0, o, ms) == E_NULL
        assert fn(ctx.handle, *shape, s, 1, 1, 0, None, ms) == E_NULL
        assert "support_order_wide" in _lib.load().jstsp_last_error().decode()
        torch.cuda.synchronize()
        assert bool((ix == -7).all()) if ms == _lib.DEVICE else np.all(hix == -7)    # (the other one is filled by its own turn)
        assert fn(ctx.handle, *shape, s, 2, 1, 0, o, ms) == 0   # and the context then orders: all zero gives 1..72 per trial
        torch.cuda.synchronize()
    want = np.tile(np.arange(1, n + 1, dtype=np.int32), 2)
    np.testing.assert_array_equal(ix.cpu().numpy(), want)
    np.testing.assert_array_equal(hix, want)


def test_python_refusals_reach_the_caller():
    S = _dev(np.zeros((GR, GT * NL), dtype=np.complex64))
    for kw in (dict(wr=-1), dict(wt=2), dict(wr=3)):
        with pytest.raises(J.JstspError, match="support_order_wide"):
            J.support_order_wide(S, GT, **kw)
    assert J.support_order_wide(S, GT).cpu().numpy().tolist() == [list(range(1, GR * GT * NL + 1))]
