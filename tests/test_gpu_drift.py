"""Frames of a tracked channel whose angles walk (jstsp_build_trials_tracked_drift_c32, csrc/inputgen.hip; build_trials(frame=,
corr=, drift=)): drift = 0 is the tracked entry and frame 0 the drawn call on the bits, the offsets are exactly linear in drift,
a frame is keyed by (seed, sweep, sequence, frame, corr, drift) and by nothing else, the channel is the float64 restatement of
tests/drift_ref.py on the returned gains and angles with the oracle's tolerances downstream, the increments have the statistics
of the model, the last accepted frame, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import drift_ref as D
from conftest import check_below, rel_err
from measured_channel_ref import reference_inputs
from oracle import system_model as osm
from test_gpu_tracking import ARRAYS, E_ARG, SENTINEL, SMALL, _same, _sp

pytestmark = pytest.mark.gpu

BIG = dict(clusters=3, rays=25, **SMALL)                     # Np = 75: 150 angles, three 64-lane blocks per sequence
SHAPES = [pytest.param(SMALL, id="Np6"), pytest.param(BIG, id="Np75")]
DPHI = ("dphi_r", "dphi_t")


def _build(p, trial0=0, batch=4, **kw):
    from jstsp19_amd.system_model import build_trials
    kw.setdefault("seed", 5)
    out = build_trials(p, trial0, batch, want_draws=True, want_H=True, **kw)
    torch.cuda.synchronize()
    return out


def _zero(out):
    for k in DPHI:
        assert out[k].dtype == torch.float64 and out[k].shape == out["u_r"].shape
        assert torch.equal(out[k], torch.zeros_like(out[k])), k


# ---- 1. the two identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", SHAPES)
def test_drift_0_is_the_tracked_entry(kw):
    p = _sp(**kw)
    for frame in (0, 1, 7):
        for corr in (0.0, 0.5, 1.0):
            a = _build(p, 3, sweep_idx=1, frame=frame, corr=corr)
            b = _build(p, 3, sweep_idx=1, frame=frame, corr=corr, drift=0.0)
            assert set(b) == set(a) | set(DPHI)
            _same(a, b)
            _zero(b)


@pytest.mark.parametrize("kw", SHAPES)
def test_frame_0_is_the_drawn_call(kw):
    p = _sp(**kw)
    drawn = _build(p, 3, sweep_idx=1)
    for corr in (0.0, 0.9):
        b = _build(p, 3, sweep_idx=1, frame=0, corr=corr, drift=0.3)
        _same(drawn, b)
        _zero(b)


# ---- 2. sum first, one multiply -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", SHAPES)
def test_offsets_are_exactly_linear_in_drift(kw):
    p = _sp(**kw)
    for f in (1, 2, 5):
        one = _build(p, frame=f, corr=0.9, drift=1.0)
        assert all(float(one[k].abs().min()) > 0 for k in DPHI)
        for s in (0.01, 0.3):
            got = _build(p, frame=f, corr=0.9, drift=s)
            for k in DPHI:
                assert torch.equal(got[k], s * one[k]), (k, f, s)
            for k in ("u_r", "u_t", "gains"):                   # the drawn angles and the tracked gains do not feel the drift
                assert torch.equal(got[k], one[k]), k
    # and the walk accumulates: frame 2's offset is frame 1's plus one more increment
    a, b = _build(p, frame=1, corr=0.9, drift=1.0), _build(p, frame=2, corr=0.9, drift=1.0)
    assert not torch.equal(a["dphi_r"], b["dphi_r"])


# ---- 3. keyed by sequence, sweep, seed and array end ------------------------------------------------------------------------------------
def _raw_call(p, batch, frame, corr, drift, memspace, *, seed=5, sweep_idx=0, trial0=0):
    """jstsp_build_trials_tracked_drift_c32 through ctypes, every output pre-filled with SENTINEL in host or device memory.
    Returns (rc, outputs as flat numpy arrays in memory order)."""
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    N, M, Gr, G2 = p.solver_shape
    Np = p.clusters * p.rays
    c64, f32 = np.complex64, np.float32
    sizes = dict(subY=(batch * N * M, c64), Omega=(batch * N * M, f32), A=(N * Gr, c64), B=(batch * G2 * M, c64),
                 Zbar=(batch * Gr * G2, c64), H=(batch * p.Nr * p.Nt * p.L, c64), indx_S=(batch * Gr * G2, np.int32),
                 gains=(batch * p.L * Np, c64), u_r=(batch * Np, f32), u_t=(batch * Np, f32), noise=(batch * p.Nr * p.T_prop, c64),
                 pilot_sym=(batch * p.Nt * p.T_prop, c64), dphi_r=(batch * Np, np.float64), dphi_t=(batch * Np, np.float64))
    host = {k: np.full(n, SENTINEL, dtype=dt) for k, (n, dt) in sizes.items()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()} if memspace == _lib.DEVICE else None
    ptr = lambda k: dev[k].data_ptr() if dev is not None else host[k].ctypes.data
    tr = _lib.Trials()
    for k in sizes:
        if k not in DPHI:
            setattr(tr, k, ptr(k))
    hyp = {k: np.full(batch, SENTINEL) for k in ("tau_Y", "tau_Z", "rho")}
    for k, v in hyp.items():
        setattr(tr, k, v.ctypes.data_as(C.POINTER(C.c_double)))
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var, _lib.BF_ZC,
                       _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    rc = ctx._lib.jstsp_build_trials_tracked_drift_c32(ctx.handle, C.byref(model), C.c_uint64(seed), sweep_idx, trial0, batch, frame,
                                                       corr, drift, C.byref(tr), ptr("dphi_r"), ptr("dphi_t"), memspace)
    torch.cuda.synchronize()
    if dev is not None:
        host = {k: v.cpu().numpy() for k, v in dev.items()}
    host.update(hyp)
    return rc, host


@pytest.mark.parametrize("kw", SHAPES)
def test_a_frame_is_keyed_by_sequence_not_by_batch(kw):
    from jstsp19_amd import _lib
    p = _sp(**kw)
    args = dict(frame=2, corr=0.7, drift=0.2)
    a = _build(p, 0, 4, **args)
    b = _build(p, 2, 2, **args)
    _same(a, b, ARRAYS + DPHI, rows=slice(2, 4))
    for other in (dict(sweep_idx=1), dict(seed=6)):
        c = _build(p, 2, 2, **args, **other)
        for k in DPHI:
            assert not torch.equal(c[k], b[k]), (k, other)
    assert not torch.equal(b["dphi_r"], b["dphi_t"])            # the two array ends walk on their own
    (rh, oh), (rd, od) = [_raw_call(p, 2, 2, 0.7, 0.2, ms, trial0=2) for ms in (_lib.HOST, _lib.DEVICE)]
    assert rh == 0 and rd == 0
    for k in oh:
        np.testing.assert_array_equal(oh[k], od[k], err_msg=k)
        assert not np.any(oh[k] == oh[k].dtype.type(SENTINEL)), k
    for k in DPHI + ("gains",):
        np.testing.assert_array_equal(od[k], b[k].cpu().numpy().reshape(-1), err_msg=k)      # and both are the wrapper's call
    np.testing.assert_array_equal(od["H"], b["H"].transpose(1, 2).contiguous().cpu().numpy().reshape(-1))
    np.testing.assert_array_equal(od["indx_S"], b["indx_S"].cpu().numpy().reshape(-1))


# ---- 4. the channel of the drifted angles, and everything after it -----------------------------------------------------------------------
@pytest.mark.parametrize("kw", SHAPES)
def test_frame_3_is_the_float64_channel_on_the_drifted_angles(kw):
    """H against channel_from_angles on the returned gains and phi_0 + dphi, the rest against the float64 restatement on that H
    and the library's own draws - the bounds of tests/test_gpu_measured_channel.py::_compare."""
    import jstsp19_amd as J
    p = _sp(**kw)
    out = _build(p, 5, 3, seed=77, sweep_idx=2, frame=3, corr=0.9, drift=0.2)
    first = _build(p, 5, 3, seed=77, sweep_idx=2, frame=0, corr=0.9, drift=0.2)
    fixed = _build(p, 5, 3, seed=77, sweep_idx=2, frame=3, corr=0.9)
    assert torch.equal(out["gains"], fixed["gains"])
    N, M, Gr, G2 = p.solver_shape
    assert torch.equal(out["u_r"], first["u_r"]) and torch.equal(out["u_t"], first["u_t"])
    assert torch.equal(J.support_order(out["Zbar"]), out["indx_S"])
    for t in range(3):
        tag = "drift.Np%d" % (p.clusters * p.rays)
        phi = [osm._laplacian(out[u][t].cpu().numpy().astype(np.float64)) + out[d][t].cpu().numpy()
               for u, d in (("u_r", "dphi_r"), ("u_t", "dphi_t"))]
        H_ref = D.channel_from_angles(out["gains"][t].cpu().numpy().astype(complex), phi[0], phi[1], p.clusters, p.rays, p.Nr, p.Nt)
        om = out["Omega"][t].cpu().numpy()
        draws = dict(noise=out["noise"][t].cpu().numpy().astype(complex), qam_idx=out["qam_idx"][t].cpu().numpy().astype(int),
                     omega_rows=np.stack([np.flatnonzero(om[:, j]) for j in range(om.shape[1])]))
        ref = reference_inputs(p, H_ref, "asis", draws)
        Hm = out["H"][t].cpu().numpy().reshape(p.Nr, p.L, p.Nt).transpose(0, 2, 1)          # columns s + Nt*l
        check_below(tag + ".H", rel_err(Hm, ref["H"]), 2e-6)
        check_below(tag + ".A", rel_err(out["A"].cpu().numpy(), ref["A"]), 2e-6)
        check_below(tag + ".B", rel_err(out["B"][t].cpu().numpy(), ref["B"]), 2e-6)
        check_below(tag + ".Zbar", rel_err(out["Zbar"][t].cpu().numpy(), ref["Zbar"]), 5e-6)
        np.testing.assert_array_equal(om, ref["Omega"])
        check_below(tag + ".subY", rel_err(out["subY"][t].cpu().numpy(), ref["subY"]), 5e-6)
        for k, tol in (("tau_Y", 2e-6), ("tau_Z", 2e-6), ("rho", 5e-5)):
            check_below(tag + "." + k, abs(float(out[k][t]) - ref[k]) / abs(ref[k]), tol)
        # the offset is not ignored: 0.2 rad per frame moves the paths by several cells of the Gr = 8 grid - against frame 0, and
        # against the same frame and gains on the fixed angles
        z3 = out["Zbar"][t].cpu().numpy().astype(complex)
        for other in (first, fixed):
            zo = other["Zbar"][t].cpu().numpy().astype(complex)
            assert np.linalg.norm(z3 - zo) > 0.1 * np.linalg.norm(zo)


# ---- 5. statistics --------------------------------------------------------------------------------------------------------------------
def _offsets_only(p, batch, frame, drift, seed=1):
    """Only dphi_* requested, through ctypes: (batch, Np) float64 each."""
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    Np = p.clusters * p.rays
    r, t = [torch.empty((batch, Np), dtype=torch.float64, device="cuda") for _ in range(2)]
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var, _lib.BF_ZC,
                       _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    tr = _lib.Trials()
    rc = ctx._lib.jstsp_build_trials_tracked_drift_c32(ctx.handle, C.byref(model), C.c_uint64(seed), 0, 0, batch, frame, 0.5, drift,
                                                       C.byref(tr), r.data_ptr(), t.data_ptr(), _lib.DEVICE)
    torch.cuda.synchronize()
    assert rc == 0
    return r, t


def test_increment_statistics_over_4096_sequences():
    """n = 4096 Np samples per frame and end.  The mean of n N(0, 1) samples has standard deviation 1/sqrt(n), their sample
    variance sqrt(2/n), the sample correlation of two independent sets 1/sqrt(n).  dphi(3) is the sum of three such increments:
    N(0, 3), whose sample variance has standard deviation 3 sqrt(2/n).  Factor 5 as in test_generator_statistics."""
    p = _sp(**SMALL)
    Np, nseq = p.clusters * p.rays, 4096
    n = nseq * Np
    d = {f: _offsets_only(p, nseq, f, 1.0) for f in (0, 1, 2, 3)}
    z = {(f, e): d[f][e] - d[f - 1][e] for f in (1, 2, 3) for e in (0, 1)}          # (nseq, Np)
    tol = 5 / np.sqrt(n)
    for k, v in z.items():
        assert abs(float(v.mean())) < tol, k
        assert abs(float((v * v).mean()) - 1.0) < 5 * np.sqrt(2.0 / n), k
    corr = lambda a, b: float((a * b).mean())
    for e in (0, 1):
        assert abs(corr(z[(1, e)], z[(2, e)])) < tol                                 # frame to frame
        assert abs(corr(z[(2, e)], z[(3, e)])) < tol
        assert abs(corr(z[(1, e)][:, :-1], z[(1, e)][:, 1:])) < tol                  # neighbouring paths
        assert abs(corr(z[(1, e)][:-1], z[(1, e)][1:])) < tol                        # neighbouring sequences
        assert abs(float((d[3][e] ** 2).mean()) - 3.0) < 3 * 5 * np.sqrt(2.0 / n)      # var(dphi(3)) = 3: three unit increments
    for f in (1, 2, 3):
        assert abs(corr(z[(f, 0)], z[(f, 1)])) < tol                                 # receive against transmit


# ---- 6. the last accepted frame ---------------------------------------------------------------------------------------------------------
def test_the_last_accepted_frame():
    p = _sp(**SMALL)
    one, s = [_build(p, batch=2, frame=65535, corr=0.25, drift=x) for x in (1.0, 0.01)]
    for k in DPHI:
        assert torch.isfinite(one[k]).all() and float(one[k].abs().min()) > 0
        assert torch.equal(s[k], 0.01 * one[k]), k
    for k in ("H", "Zbar", "subY"):
        assert torch.isfinite(torch.view_as_real(s[k])).all(), k


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,corr,drift", [(1, 0.5, -0.1), (1, 0.5, float("nan")), (1, 0.5, float("inf")), (1, 1.5, 0.1),
                                              (65536, 0.5, 0.1)])
def test_bad_arguments_are_refused_and_nothing_is_written(frame, corr, drift):
    from jstsp19_amd import _lib
    p = _sp(**SMALL)
    for ms in (_lib.DEVICE, _lib.HOST):
        rc, o = _raw_call(p, 2, frame, corr, drift, ms)
        assert rc == E_ARG
        assert "build_trials_tracked" in _lib.load().jstsp_last_error().decode()
        for k, v in o.items():
            assert np.all(v == v.dtype.type(SENTINEL)), k
    drawn = _build(p)
    b = _build(p, frame=0, corr=0.5, drift=0.1)                 # the context then builds frame 0 correctly
    _same(drawn, b)
    _zero(b)
