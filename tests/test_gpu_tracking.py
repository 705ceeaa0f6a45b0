"""Frames of a time-varying channel built on the device (jstsp_build_trials_tracked_c32, csrc/inputgen.hip; build_trials(frame=,
corr=)) and the tracking sweep on them (montecarlo.run_tracking): frame 0 is the drawn call on the bits, corr = 1 a static channel,
the gains follow the float64 recursion of tests/tracking_ref.py on the library's own innovations, everything downstream of the
channel matches the oracle on the library's own draws, a frame is keyed by (seed, sweep, sequence, frame, corr) and by nothing
else, the statistics of the model, the refusals, and the runner against its own loop restated here."""
import ctypes as C

import numpy as np
import pytest
import torch

import tracking_ref as R
from conftest import check_below, rel_err

pytestmark = pytest.mark.gpu

ARRAYS = ("subY", "Omega", "A", "B", "Zbar", "indx_S", "H", "gains", "u_r", "u_t", "noise", "qam_idx", "pilot_sym", "tau_Y", "tau_Z",
          "rho")
SMALL = dict(Nt=2, Nr=8, L=2, T=4, Mr=2)                    # the shape of test_draws_are_keyed_by_trial_not_by_batch
SENTINEL = -777.0
E_ARG = -4


def _sp(**kw):
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(**kw)


def _build(p, trial0=0, batch=4, **kw):
    from jstsp19_amd.system_model import build_trials
    kw.setdefault("seed", 5)
    out = build_trials(p, trial0, batch, want_draws=True, want_H=True, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, keys=ARRAYS, rows=slice(None)):
    for k in keys:
        x = a[k] if k == "A" else a[k][rows]
        assert torch.equal(x, b[k]), k


# ---- 1. frame 0 is the drawn call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(shared_pilots=True), dict(pilots="gauss")])
def test_frame_0_is_the_drawn_call(opts):
    p = _sp(**SMALL)
    drawn = _build(p, 3, sweep_idx=1, **opts)
    assert set(ARRAYS) <= set(drawn)
    for corr in (0.0, 0.5, 1.0):
        _same(drawn, _build(p, 3, sweep_idx=1, frame=0, corr=corr, **opts))


# ---- 2. a static channel -----------------------------------------------------------------------------------------------------------
def test_corr_1_keeps_the_channel_and_redraws_the_frame():
    p = _sp(**SMALL)
    f0, f1, f7 = [_build(p, frame=f, corr=1.0) for f in (0, 1, 7)]
    for f in (f1, f7):
        _same(f0, f, ("gains", "u_r", "u_t", "H", "Zbar", "indx_S"))
    for a, b in ((f0, f1), (f0, f7), (f1, f7)):
        for k in ("noise", "qam_idx", "Omega", "subY"):
            assert not torch.equal(a[k], b[k]), k


# ---- 3. the recursion ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def innovations():
    """w_0 .. w_5 of sequences [0, 4): frame k at corr = 0 returns the innovation w_k.  Also frame 0's u_r, u_t."""
    p = _sp(**SMALL)
    outs = [_build(p, frame=k, corr=0.0) for k in range(6)]
    w = np.stack([o["gains"].cpu().numpy() for o in outs])
    assert w.dtype == np.complex64 and w.shape == (6, 4, p.L, p.clusters * p.rays)
    assert len({w[k].tobytes() for k in range(6)}) == 6
    return p, w, outs[0]["u_r"].clone(), outs[0]["u_t"].clone()


@pytest.mark.parametrize("corr", [0.3, 0.95])
@pytest.mark.parametrize("frame", [1, 2, 5])
def test_gains_follow_the_recursion(innovations, corr, frame):
    """One rounding to fp32 is 2^-24 relative per component; the bound allows a factor 2 over it."""
    p, w, u_r, u_t = innovations
    out = _build(p, frame=frame, corr=corr)
    ref = R.gain_at(w, corr, frame)
    g = out["gains"].cpu().numpy().astype(np.complex128)
    diff = max(np.max(np.abs(g.real - ref.real)), np.max(np.abs(g.imag - ref.imag)))
    check_below("tracking_gains_vs_recursion", diff / np.max(np.abs(ref)), 2.0 ** -23)
    assert torch.equal(out["u_r"], u_r) and torch.equal(out["u_t"], u_t)


def test_the_last_accepted_frame():
    """Frame 65535 at corr = 0.25: the weight of w_{65535-j} is sqrt(15/16) 4^-j, so the 41 last innovations carry the gain and
    what the recursion started at frame 65495 leaves out is below 4^-40 < 1e-24 - far under the one fp32 rounding the bound is for."""
    p = _sp(**SMALL)
    last, n = 65535, 41
    w = np.stack([_build(p, batch=2, frame=last - n + 1 + j, corr=0.0)["gains"].cpu().numpy() for j in range(n)])
    ref = R.gain_at(np.concatenate([np.zeros_like(w[:1]), w]), 0.25, n)          # g = 0 before the first of them
    g = _build(p, batch=2, frame=last, corr=0.25)["gains"].cpu().numpy().astype(np.complex128)
    diff = max(np.max(np.abs(g.real - ref.real)), np.max(np.abs(g.imag - ref.imag)))
    check_below("tracking_gains_vs_recursion_frame_65535", diff / np.max(np.abs(ref)), 2.0 ** -23)


# ---- 4. downstream of the channel, against the oracle on the library's own draws ---------------------------------------------------
@pytest.mark.parametrize("kw", [dict(Nt=4, Nr=16, L=3, T=6, Mr=4, snr_db=5.0),
                                dict(Nt=2, Nr=12, L=2, T=7, Mr=3, Mr_e=9, Gr=16, Gt=4, clusters=3, rays=2, snr_db=10.0)])
def test_frame_3_matches_the_oracle_on_its_own_draws(kw):
    """The tolerances are those of test_gpu_inputgen.py::test_build_trials_matches_oracle_on_its_own_draws."""
    from test_gpu_inputgen import _oracle_inputs
    p = _sp(**kw)
    out = _build(p, 5, 3, seed=77, sweep_idx=2, frame=3, corr=0.9)
    drawn = _build(p, 5, 3, seed=77, sweep_idx=2)
    assert not torch.equal(out["gains"], drawn["gains"]) and torch.equal(out["u_r"], drawn["u_r"])
    N, M, Gr, G2 = p.solver_shape
    assert out["subY"].stride() == (N * M, 1, N) and out["B"].stride() == (G2 * M, 1, G2)
    for t in range(3):
        ref, _ = _oracle_inputs(p, out, t)
        Hm = out["H"][t].cpu().numpy().reshape(p.Nr, p.L, p.Nt).transpose(0, 2, 1)     # columns s + Nt*l
        assert rel_err(Hm, ref["H"]) < 2e-6
        assert rel_err(out["Zbar"][t].cpu().numpy(), ref["Zbar"]) < 5e-6
        np.testing.assert_array_equal(out["Omega"][t].cpu().numpy(), ref["Omega"])
        assert rel_err(out["subY"][t].cpu().numpy(), ref["subY"]) < 5e-6
        assert rel_err(out["A"].cpu().numpy(), ref["A"]) < 2e-6
        assert rel_err(out["B"][t].cpu().numpy(), ref["B"]) < 2e-6
        np.testing.assert_allclose(float(out["tau_Y"][t]), ref["tau_Y"], rtol=2e-6)
        np.testing.assert_allclose(float(out["tau_Z"][t]), ref["tau_Z"], rtol=2e-6)
        np.testing.assert_allclose(float(out["rho"][t]), ref["rho"], rtol=5e-5)
        ix = out["indx_S"][t].cpu().numpy().astype(np.int64) - 1
        assert np.array_equal(np.sort(ix), np.arange(Gr * G2))
        mag = np.abs(ref["Zbar"].reshape(-1, order="F"))[ix]
        assert np.all(np.diff(mag) <= 2e-6 * mag[0])
        np.testing.assert_array_equal(ix[:10] + 1, ref["indx_S"][:10])


# ---- 5. keyed by sequence, not by batch ----------------------------------------------------------------------------------------------
def _raw_call(p, batch, frame, corr, memspace, *, seed=5, sweep_idx=0, trial0=0):
    """jstsp_build_trials_tracked_c32 through ctypes, the outputs pre-filled with SENTINEL in host or device memory.  Returns
    (rc, outputs as flat numpy arrays in memory order)."""
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    N, M, Gr, G2 = p.solver_shape
    Np = p.clusters * p.rays
    c64, f32 = np.complex64, np.float32
    sizes = dict(subY=(batch * N * M, c64), Omega=(batch * N * M, f32), A=(N * Gr, c64), B=(batch * G2 * M, c64),
                 Zbar=(batch * Gr * G2, c64), H=(batch * p.Nr * p.Nt * p.L, c64), indx_S=(batch * Gr * G2, np.int32),
                 gains=(batch * p.L * Np, c64), u_r=(batch * Np, f32), u_t=(batch * Np, f32), noise=(batch * p.Nr * p.T_prop, c64),
                 pilot_sym=(batch * p.Nt * p.T_prop, c64))
    host = {k: np.full(n, SENTINEL, dtype=dt) for k, (n, dt) in sizes.items()}
    if memspace == _lib.DEVICE:
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    tr = _lib.Trials()
    for k in sizes:
        setattr(tr, k, dev[k].data_ptr() if memspace == _lib.DEVICE else host[k].ctypes.data)
    hyp = {k: np.full(batch, SENTINEL) for k in ("tau_Y", "tau_Z", "rho")}
    for k, v in hyp.items():
        setattr(tr, k, v.ctypes.data_as(C.POINTER(C.c_double)))
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 0, p.noise_var, _lib.BF_ZC,
                       _lib.RHO_MIN6, 1.0, _lib.PILOTS_QAM4)
    rc = ctx._lib.jstsp_build_trials_tracked_c32(ctx.handle, C.byref(model), C.c_uint64(seed), sweep_idx, trial0, batch, frame, corr,
                                                 C.byref(tr), memspace)
    torch.cuda.synchronize()
    if memspace == _lib.DEVICE:
        host = {k: v.cpu().numpy() for k, v in dev.items()}
    host.update(hyp)
    return rc, host


def test_a_frame_is_keyed_by_sequence_not_by_batch():
    from jstsp19_amd import _lib
    p = _sp(**SMALL)
    a = _build(p, 0, 4, frame=2, corr=0.7)
    b = _build(p, 2, 2, frame=2, corr=0.7)
    _same(a, b, rows=slice(2, 4))
    assert not torch.equal(_build(p, 2, 2, frame=2, corr=0.7, sweep_idx=1)["gains"], b["gains"])
    assert not torch.equal(_build(p, 2, 2, frame=2, corr=0.7, seed=6)["gains"], b["gains"])
    (rh, oh), (rd, od) = [_raw_call(p, 2, 2, 0.7, ms, trial0=2) for ms in (_lib.HOST, _lib.DEVICE)]
    assert rh == 0 and rd == 0
    for k in oh:
        np.testing.assert_array_equal(oh[k], od[k], err_msg=k)
        assert not np.any(oh[k] == oh[k].dtype.type(SENTINEL)), k
    np.testing.assert_array_equal(od["gains"], b["gains"].cpu().numpy().reshape(-1))        # and both are the wrapper's call
    np.testing.assert_array_equal(od["H"], b["H"].transpose(1, 2).contiguous().cpu().numpy().reshape(-1))
    np.testing.assert_array_equal(od["subY"], b["subY"].transpose(1, 2).contiguous().cpu().numpy().reshape(-1))


# ---- 6. statistics ---------------------------------------------------------------------------------------------------------------------
def test_gain_statistics_over_4096_sequences():
    """n = 4096 L Np complex samples per frame.  |g|^2 of a CN(0, 1) sample has variance 1; the product g_a conj(g_b) of two
    CN(0, 1) samples of correlation r has a real part of variance (1 + r^2)/2 and an imaginary part of variance (1 - r^2)/2 (bounded
    by the same figure).  Factor 5 as in test_generator_statistics."""
    from jstsp19_amd.system_model import build_trials
    p = _sp(clusters=1, rays=2, **SMALL)
    g = {}
    for f in (0, 1, 3):
        g[f] = build_trials(p, 0, 4096, seed=1, frame=f, corr=0.8, want_draws=True)["gains"].to(torch.complex128).reshape(-1)
    n = g[0].numel()
    assert n == 4096 * p.L * 2
    for f in g:
        assert abs(float((g[f].abs() ** 2).mean()) - 1.0) < 5 / np.sqrt(n), f
    for f, e in ((1, 0), (3, 1), (3, 0)):
        r = 0.8 ** (f - e)
        c = complex((g[f] * g[e].conj()).mean())
        tol = 5 * np.sqrt((1 + r * r) / (2 * n))
        assert abs(c.real - r) < tol and abs(c.imag) < tol, (f, e, c)
    per_seq = p.L * 2
    for f in g:                                                 # sequence t against sequence t + 1: independent
        c = complex((g[f] * torch.roll(g[f], per_seq).conj()).mean())
        assert abs(c.real) < 5 / np.sqrt(2 * n) and abs(c.imag) < 5 / np.sqrt(2 * n), (f, c)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,corr", [(1, -0.1), (1, 1.5), (1, float("nan")), (-1, 0.5), (65536, 0.5)])
def test_bad_corr_and_frame_are_refused_and_nothing_is_written(frame, corr):
    from jstsp19_amd import _lib
    p = _sp(**SMALL)
    for ms in (_lib.DEVICE, _lib.HOST):
        rc, o = _raw_call(p, 2, frame, corr, ms)
        assert rc == E_ARG
        assert "build_trials_tracked" in _lib.load().jstsp_last_error().decode()
        for k, v in o.items():
            assert np.all(v == v.dtype.type(SENTINEL)), k
    _same(_build(p), _build(p, frame=0, corr=0.5))              # the context then builds frame 0 correctly


# ---- 8. the runner -------------------------------------------------------------------------------------------------------------------
TOOL_KEYS = {"tool", "precision", "shape", "frames", "seqs", "corr", "clusters", "rays", "snr_db", "seed", "scored_frames", "cold_imax",
             "results", "channel"}
RESULT_KEYS = {"mode", "Imax", "mean_nmse", "sem_over_seqs", "median_nmse", "mean_nmse_by_frame", "estimates_per_s"}


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_run_tracking_on_a_static_channel(precision):
    import jstsp19_amd as J
    from jstsp19_amd.montecarlo import run_tracking
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=2, Nr=8, L=2, T=6, Mr=2)
    kw = dict(imax=(3,), cold_imax=6, precision=precision, seed=11, sweep_idx=2)
    res = run_tracking(p, 4, 3, 1.0, batch=4, **kw)
    assert set(res) == TOOL_KEYS and res["channel"] == "device" and res["tool"] == "run_tracking"
    assert res["scored_frames"] == [1, 2] and res["frames"] == 3 and res["seqs"] == 4 and res["corr"] == 1.0
    assert res["shape"] == list(p.solver_shape) and res["precision"] == precision and res["cold_imax"] == 6
    got = {(r["mode"], r["Imax"]): r for r in res["results"]}
    assert list(got) == [("cold", 3), ("cold", 6), ("warm", 3), ("warm_vs", 3)]
    for r in got.values():
        assert set(r) == RESULT_KEYS and len(r["mean_nmse_by_frame"]) == 2 and r["estimates_per_s"] > 0
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in r["mean_nmse_by_frame"])
    strip = lambda d: [{k: v for k, v in r.items() if k != "estimates_per_s"} for r in d["results"]]
    assert strip(run_tracking(p, 4, 3, 1.0, batch=4, **kw)) == strip(res)                  # a repeated call: the same floats

    # the cold columns, restated: frames from build_trials, each solved from zero and scored
    f64 = precision == "f64"
    wide = (lambda x: J.colmajor(x.to(torch.complex128))) if f64 else (lambda x: x)
    solve = J.proposed_algorithm_resume_f64 if f64 else J.proposed_algorithm_resume
    score = J.nmse_spectral_f64 if f64 else J.nmse_spectral
    want = {3: [], 6: []}
    for f in (1, 2):
        inp = build_trials(p, 0, 4, seed=11, sweep_idx=2, frame=f, corr=1.0)
        args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)) if f64 else inp["Omega"], wide(inp["A"]), wide(inp["B"]))
        for n_it in want:
            S = solve(*args, n_it, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy(), want_ce=False,
                      return_state=False)[0]
            want[n_it].append(torch.as_tensor(score(S, wide(inp["Zbar"]))).double().cpu().numpy())
    for n_it, e in want.items():
        ref = [float(x) for x in np.stack(e).mean(axis=1)]
        if f64:
            assert got[("cold", n_it)]["mean_nmse_by_frame"] == ref
        else:
            np.testing.assert_allclose(got[("cold", n_it)]["mean_nmse_by_frame"], ref, rtol=1e-5)

    # chunks of 3 + 1 sequences: the frames are keyed by sequence, so only the solver's batch changes (float64: rounding level)
    if f64:
        chunked = run_tracking(p, 4, 3, 1.0, batch=3, **kw)
        for a, b in zip(strip(chunked), strip(res)):
            np.testing.assert_allclose(a["mean_nmse_by_frame"], b["mean_nmse_by_frame"], rtol=1e-9)
