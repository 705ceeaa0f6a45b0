"""Capacity / energy-efficiency path on the device (csrc/capacity.hip): the codebooks of createBeamformer.m, the batched ASE of
plot_capacity.m on given inputs against float64 on the same values, and the device-built sweep against float64 ASE of
jstsp_build_trials_c32's own channel and pilots for the same trials, plus the statistics of the sweep against a numpy run of
the reference's samplers (tests/capacity_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import capacity_ref as R
from conftest import check_below

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ZC", "fft", "ps", "quantized", "quantized_4")


def _rand(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 0.3


def _ref(Y, W, cols, scale):
    """float64 ASE per problem on the operand values the device saw (cols: (batch, Mr) 1-based)."""
    Y = np.asarray(Y, dtype=np.complex128)
    W = np.asarray(W, dtype=np.complex128)
    return np.array([R.ase_chol(Y[t], W[:, np.asarray(cols[t]) - 1], scale) for t in range(Y.shape[0])])


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))


@pytest.mark.parametrize("N", [1, 7, 32, 64, 100, 128, 256])
def test_beamformer_codebooks(N):
    import jstsp19_amd as J
    for kind in KINDS:
        ref = R.create_beamformer(N, kind)
        W = J.beamformer(N, kind)
        check_below("bf_c32_abs_times_sqrtN", np.max(np.abs(W - ref)) * np.sqrt(N), 1e-6)
        W64 = J.beamformer(N, kind, dtype=np.complex128)
        # the float64 transcription evaluates exp() of unreduced phases (up to 11 pi N): its own error grows like N eps
        check_below("bf_c64_abs_times_sqrtN_over_N", np.max(np.abs(W64 - ref)) * np.sqrt(N) / N, 4e-14)
        Wd = J.beamformer(N, kind, device="cuda:0")
        torch.cuda.synchronize()
        assert np.array_equal(Wd.cpu().numpy(), W)


SHAPES = [  # Nr, T, Ncols, Mr, batch
    (32, 20, 32, 7, 3),        # Mr < T
    (64, 5, 64, 22, 5),        # Mr > T
    (32, 5, 32, 1, 2),         # Mr = 1
    (128, 5, 128, 128, 3),     # Mr = Ncols (DBF at Nr = 128)
    (64, 1, 64, 16, 7),        # T = 1, odd batch
    (96, 64, 96, 70, 2),       # n = 64 on the T side
    (64, 100, 80, 64, 1),      # n = 64 on the Mr side, several chunks of q
    (48, 7, 40, 33, 5),        # Ncols < Nr, odd batch
]


@pytest.mark.parametrize("Nr,T,Ncols,Mr,batch", SHAPES)
def test_ase_given_inputs_against_float64(Nr, T, Ncols, Mr, batch):
    import jstsp19_amd as J
    rng = np.random.default_rng(Nr * 1000 + T * 10 + Mr)
    Y = _rand(rng, batch, Nr, T).astype(np.complex64)
    W = _rand(rng, Nr, Ncols).astype(np.complex64)
    first = np.tile(np.arange(1, Mr + 1), (batch, 1))
    ref = _ref(Y, W, first, R.SCALE)
    a = J.ase(Y, W, R.SCALE, Mr=Mr)
    check_below("ase_c32_rel", _rel(a, ref), 1e-13)
    # duplicated columns, per-problem subsets
    cols = rng.integers(1, Ncols + 1, size=(batch, Mr)).astype(np.int32)
    cols[:, -1] = cols[:, 0]
    check_below("ase_c32_rel", _rel(J.ase(Y, W, R.SCALE, cols=cols), _ref(Y, W, cols, R.SCALE)), 1e-13)
    # the device memspace gives the same bits
    dev = torch.device("cuda:0")
    Yd = J.colmajor(torch.from_numpy(Y).to(dev))
    Wd = J.colmajor(torch.from_numpy(W).to(dev))
    ad = J.ase(Yd, Wd, R.SCALE, cols=torch.from_numpy(first.astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    assert np.array_equal(ad.cpu().numpy(), a)                       # explicit 1..Mr on the device = NULL on the host


def test_ase_exact_and_bad_cases():
    import jstsp19_amd as J
    rng = np.random.default_rng(5)
    W = J.beamformer(64, "ZC")
    Y = _rand(rng, 5, 64, 5).astype(np.complex64)
    assert np.array_equal(J.ase(np.zeros((3, 64, 5), np.complex64), W, R.SCALE, Mr=9), np.zeros(3))    # Y = 0: 0 exactly
    a = J.ase(Y, W, R.SCALE, Mr=12)
    assert np.array_equal(J.ase(Y, W, R.SCALE, cols=np.tile(np.arange(1, 13), (5, 1))), a)           # NULL = 1..Mr, same bits
    with pytest.raises(J.JstspError) as e:                                                           # n = 65
        J.ase(_rand(rng, 1, 80, 65).astype(np.complex64), J.beamformer(80, "ZC"), R.SCALE, Mr=65)
    assert e.value.code == -3
    cols = np.tile(np.arange(1, 13), (5, 1)).astype(np.int32)
    cols[1, 4] = 0
    cols[3, 0] = 65
    b = J.ase(Y, W, R.SCALE, cols=cols)
    assert np.isnan(b[1]) and np.isnan(b[3])
    assert np.array_equal(b[[0, 2, 4]], a[[0, 2, 4]])
    # prefixes of a fixed codebook on one Y: non-decreasing in Mr (interlacing)
    y = _rand(rng, 1, 64, 5).astype(np.complex64)
    pre = np.array([J.ase(y, W, R.SCALE, Mr=m)[0] for m in range(1, 65)])
    assert np.all(np.diff(pre) >= -1e-12 * pre[1:])
    # 'quantized' at N = 64 is the unitary DFT: all 64 columns give log2 det(I + c Y^H Y) (to the fp32 rounding of W)
    Yq = _rand(rng, 4, 64, 5).astype(np.complex64)
    full = J.ase(Yq, J.beamformer(64, "quantized"), R.SCALE, Mr=64)
    direct = np.array([np.linalg.slogdet(np.eye(5) + R.SCALE * Yq[t].astype(complex).conj().T @ Yq[t])[1] / np.log(2)
                       for t in range(4)])
    check_below("ase_quantized64_unitary_rel", _rel(full, direct), 3e-8)


def test_ase_c64_against_float64():
    import jstsp19_amd as J
    rng = np.random.default_rng(11)
    for Nr, T, Ncols, Mr, batch in SHAPES[:5]:
        Y = _rand(rng, batch, Nr, T)
        W = R.create_beamformer(Ncols, "ZC")[:Nr] if Ncols == Nr else _rand(rng, Nr, Ncols)
        cols = rng.integers(1, Ncols + 1, size=(batch, Mr)).astype(np.int32)
        check_below("ase_c64_rel", _rel(J.ase(Y, W, R.SCALE, cols=cols), _ref(Y, W, cols, R.SCALE)), 1e-14)


def _sweep_vs_build_trials(panel, Mr, trial0, batch, seed, sweep_idx):
    import jstsp19_amd as J
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import ase_trials, build_trials
    p = [q for q in M.capacity_points(panel) if q.Mr == Mr][0]
    a, cols = ase_trials(p, M.capacity_designs(p), trial0, batch, seed=seed, sweep_idx=sweep_idx, want_cols=True)
    inp = build_trials(p, trial0, batch, seed=seed, sweep_idx=sweep_idx, want_H=True, want_draws=True)
    torch.cuda.synchronize()
    a, cols = a.cpu().numpy(), cols.cpu().numpy()
    H, ps = inp["H"].cpu().numpy().astype(complex), inp["pilot_sym"].cpu().numpy().astype(complex)
    W_zc = J.beamformer(p.Nr, "ZC").astype(complex)
    W_q = J.beamformer(p.Nr, "quantized").astype(complex)
    ref = np.array([R.designs_ase(R.received(H[t], ps[t]), p.Nr, Mr, cols[t] - 1, W_zc, W_q) for t in range(batch)])
    return a, cols, ref


@pytest.mark.parametrize("panel", [1, 2, 3])
def test_device_sweep_against_float64_of_build_trials(panel):
    for Mr in (1, 4, 13, 31):
        a, cols, ref = _sweep_vs_build_trials(panel, Mr, 3, 24, 20190913, 5)
        assert cols.shape == (24, Mr)
        check_below("ase_trials_rel", _rel(a, ref), 2e-12)
        assert np.all(a[:, 0] >= a[:, 2] * (1 - 1e-12))                  # DBF >= HBF-ZC per trial
        assert np.all(np.isfinite(a)) and np.all(a > 0)


def test_device_sweep_does_not_depend_on_the_batch():
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import ase_trials
    p = M.capacity_points(3)[4]
    d = M.capacity_designs(p)
    big, cb = ase_trials(p, d, 0, 40, seed=3, sweep_idx=2, want_cols=True)
    small, cs = ase_trials(p, d, 5, 7, seed=3, sweep_idx=2, want_cols=True)
    torch.cuda.synchronize()
    assert torch.equal(big[5:12], small) and torch.equal(cb[5:12], cs)


def test_proposed_subsets_are_uniform():
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import ase_trials
    p = [q for q in M.capacity_points(3) if q.Mr == 13][0]
    n = 4096
    _, cols = ase_trials(p, M.capacity_designs(p), 0, n, seed=17, sweep_idx=1, want_cols=True)
    cols = cols.cpu().numpy()
    assert cols.min() >= 1 and cols.max() <= p.Mr_e
    assert all(len(set(r)) == p.Mr for r in cols)
    q = p.Mr / p.Mr_e
    count = np.bincount(cols.reshape(-1), minlength=p.Mr_e + 1)[1:]
    assert np.all(np.abs(count - n * q) <= 5 * np.sqrt(n * q * (1 - q))), count


def test_panel1_statistics_against_the_reference_samplers():
    from jstsp19_amd import montecarlo as M
    pts = [q for q in M.capacity_points(1) if q.Mr in (1, 13, 31)]
    n = 2000
    mean, se = M.run_capacity(pts, n, batch=2000, seed=20190913, sweep0=900)
    rng = np.random.default_rng(20190913)
    for i, p in enumerate(pts):
        x = R.monte_carlo(p.Nr, p.Mr_e, p.Mr, n, rng)
        mn, sn = x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(n)
        z = np.abs(mean[i] - mn) / np.sqrt(se[i] ** 2 + sn ** 2)
        check_below("capacity_panel1_z", float(np.max(z)), 4.0)


def test_run_capacity_driver_ee():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_capacity.py"), "--figure", "ee", "--trials", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if l.split() and l.split()[0].isdigit()]
    assert [int(x[0]) for x in rows] == list(range(1, 33, 3))
    for x in rows:
        v = np.array([float(s) for s in x[1:]])
        ase, power, ee = v[0:4], v[4:8], v[8:12]
        assert np.allclose(power, R.power_model(64, int(x[0]), 32), rtol=1e-6)
        assert np.allclose(ee, ase / power, rtol=1e-5)
    assert "wall" in r.stdout


def test_ase_cols_must_live_where_Y_lives():
    """The library reads cols in the call's memspace: a host index array with device Y / W (or the reverse) is refused in
    Python before anything is launched."""
    import jstsp19_amd as J
    rng = np.random.default_rng(2)
    Y = _rand(rng, 3, 32, 5).astype(np.complex64)
    W = J.beamformer(32, "ZC")
    dev = torch.device("cuda:0")
    Yd, Wd = J.colmajor(torch.from_numpy(Y).to(dev)), J.colmajor(torch.from_numpy(W).to(dev))
    cols = np.tile(np.arange(1, 5, dtype=np.int32), (3, 1))
    with pytest.raises(ValueError):
        J.ase(Yd, Wd, R.SCALE, cols=cols)                                  # numpy cols, device Y
    with pytest.raises(ValueError):
        J.ase(Yd, Wd, R.SCALE, cols=torch.from_numpy(cols))                # CPU tensor, device Y
    with pytest.raises(ValueError):
        J.ase(Yd, Wd, R.SCALE, cols=torch.from_numpy(cols).to(dev).long())  # not int32
    with pytest.raises(ValueError):
        J.ase(Y, W, R.SCALE, cols=torch.from_numpy(cols).to(dev))          # device cols, host Y
    with pytest.raises(ValueError):
        J.ase(Y, W, R.SCALE, cols=torch.from_numpy(cols))                  # a tensor with host Y


@pytest.mark.parametrize("Mr", [1, 3, 12])
def test_ase_non_finite_input_gives_nan_for_its_trial(Mr):
    import jstsp19_amd as J
    rng = np.random.default_rng(8)
    W = J.beamformer(64, "quantized")
    Y = _rand(rng, 5, 64, 5).astype(np.complex64)
    clean = J.ase(Y, W, R.SCALE, Mr=Mr)
    Y[1, 7, 2] = np.inf
    Y[3, 0, 0] = complex(np.nan, 0.0)
    Y[4, 5, 4] = complex(0.0, -np.inf)
    for Yx in (Y, Y.astype(np.complex128)):
        a = J.ase(Yx, W.astype(Yx.dtype), R.SCALE, Mr=Mr)
        assert np.isnan(a[1]) and np.isnan(a[3]) and np.isnan(a[4])
        if Yx.dtype == np.complex64:
            assert np.array_equal(a[[0, 2]], clean[[0, 2]])


def test_device_sweep_host_memspace_gives_the_device_bits():
    """jstsp_ase_trials_c32 with host output arrays (the C ABI's JSTSP_HOST memspace) returns the bits of the device call."""
    import ctypes as C
    from jstsp19_amd import _lib, montecarlo as M
    from jstsp19_amd.solvers import _bf_kind
    from jstsp19_amd.system_model import ase_trials
    p = M.capacity_points(2)[5]
    d = M.capacity_designs(p)
    dev_a, dev_c = ase_trials(p, d, 11, 33, seed=9, sweep_idx=4, want_cols=True)
    torch.cuda.synchronize()
    c = _lib.Context(0)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var,
                       _lib.BF_ZC, _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    ds = (_lib.AseDesign * len(d))(*[_lib.AseDesign(_bf_kind(k), n, pool) for k, n, pool in d])
    a = np.full((33, len(d)), -1.0)
    cols = np.zeros((33, p.Mr), dtype=np.int32)
    _lib.check(c._lib.jstsp_ase_trials_c32(c.handle, C.byref(model), ds, len(d), C.c_uint64(9), 4, 11, 33, a.ctypes.data,
                                           cols.ctypes.data, _lib.HOST), "jstsp_ase_trials_c32")
    c.close()
    assert np.array_equal(a, dev_a.cpu().numpy()) and np.array_equal(cols, dev_c.cpu().numpy())


@pytest.mark.parametrize("pilots,shared", [("gauss", False), ("qam4", True)])
def test_device_sweep_follows_the_pilot_options_of_build_trials(pilots, shared):
    import jstsp19_amd as J
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import ase_trials, build_trials
    p = [q for q in M.capacity_points(1) if q.Mr == 13][0]
    a, cols = ase_trials(p, M.capacity_designs(p), 2, 16, seed=5, sweep_idx=6, want_cols=True, pilots=pilots,
                         shared_pilots=shared)
    inp = build_trials(p, 2, 16, seed=5, sweep_idx=6, want_H=True, want_draws=True, pilots=pilots, shared_pilots=shared)
    torch.cuda.synchronize()
    a, cols = a.cpu().numpy(), cols.cpu().numpy()
    ps = inp["pilot_sym"].cpu().numpy()
    if pilots == "gauss":
        ps = ps * np.float32(0.70710678)               # ...training.m:20, in fp32 as the pilot kernels scale them
    if shared:
        assert np.array_equal(ps[0], ps[-1])
    H, ps = inp["H"].cpu().numpy().astype(complex), ps.astype(complex)
    W_zc, W_q = J.beamformer(p.Nr, "ZC").astype(complex), J.beamformer(p.Nr, "quantized").astype(complex)
    ref = np.array([R.designs_ase(R.received(H[t], ps[t]), p.Nr, p.Mr, cols[t] - 1, W_zc, W_q) for t in range(16)])
    check_below("ase_trials_rel", _rel(a, ref), 2e-12)
