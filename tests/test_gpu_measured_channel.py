"""jstsp_build_trials_from_channel_c32 (csrc/inputgen.hip): the builder on a channel the caller supplies - the first lines of
plot_errorVSsnr_nyuwireless.m (:60-69) - against the drawn path (same bits), against the float64 restatement of
tests/measured_channel_ref.py at the tolerances of tests/test_gpu_inputgen.py, on spectra that stress the Jacobi behind
sigma_max, in both memspaces, its refusals, and through the solvers and the sweep runner."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import TOL_S, check_below, rel_err
from measured_channel_ref import cut_and_scale, make_channel, reference_inputs

pytestmark = pytest.mark.gpu

MODES = ("asis", "reference", "unit")
TOL_SIGMA = 1e-12           # the bound the float64 Jacobi paths meet elsewhere


def _sp(**kw):
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(**kw)


def _c64(H):
    """What the device sees: the channel narrowed once to complex64."""
    return np.asarray(H).astype(np.complex64)


def _compare(tag, p, out, src, mode, t, with_hbf):
    """Trial t of ``out`` against the float64 restatement on the same channel and the library's own draws."""
    om = out["Omega"][t].cpu().numpy()
    rows = np.stack([np.flatnonzero(om[:, j]) for j in range(om.shape[1])])
    draws = dict(noise=out["noise"][t].cpu().numpy().astype(complex), qam_idx=out["qam_idx"][t].cpu().numpy().astype(int),
                 omega_rows=rows)
    ref = reference_inputs(p, src.astype(complex), mode, draws, with_hbf=with_hbf)
    N, M, Gr, G2 = p.solver_shape
    Hm = out["H"][t].cpu().numpy().reshape(p.Nr, p.L, p.Nt).transpose(0, 2, 1)          # columns s + Nt*l
    check_below(tag + ".H", rel_err(Hm, ref["H"]), 2e-6)
    check_below(tag + ".A", rel_err(out["A"].cpu().numpy(), ref["A"]), 2e-6)
    check_below(tag + ".B", rel_err(out["B"][t].cpu().numpy(), ref["B"]), 2e-6)
    check_below(tag + ".Zbar", rel_err(out["Zbar"][t].cpu().numpy(), ref["Zbar"]), 5e-6)
    np.testing.assert_array_equal(om, ref["Omega"])
    check_below(tag + ".subY", rel_err(out["subY"][t].cpu().numpy(), ref["subY"]), 5e-6)
    for k, tol in (("tau_Y", 2e-6), ("tau_Z", 2e-6), ("rho", 5e-5)):
        check_below(tag + "." + k, abs(float(out[k][t]) - ref[k]) / abs(ref[k]), tol)
    ix = out["indx_S"][t].cpu().numpy().astype(np.int64) - 1
    assert np.array_equal(np.sort(ix), np.arange(Gr * G2))
    mag = np.abs(ref["Zbar"].reshape(-1, order="F"))[ix]
    assert np.all(np.diff(mag) <= 2e-6 * mag[0])
    np.testing.assert_array_equal(ix[:10] + 1, ref["indx_S"][:10])
    if with_hbf:
        check_below(tag + ".Y_hbf", rel_err(out["Y_hbf"][t].cpu().numpy(), ref["Y_hbf"]), 5e-6)
        check_below(tag + ".A_hbf", rel_err(out["A_hbf"].cpu().numpy(), ref["A_hbf"]), 2e-6)
        check_below(tag + ".B_hbf", rel_err(out["B_hbf"][t].cpu().numpy(), ref["B_hbf"]), 2e-6)
    return ref


def _check_sigma(tag, p, out, src):
    sig = out["sigma_max"].numpy().reshape(-1, p.L)
    chans = src.reshape((-1,) + src.shape[-3:])
    assert sig.shape[0] == chans.shape[0]
    for c in range(chans.shape[0]):
        want = cut_and_scale(p, chans[c].astype(complex), "asis")[1]
        check_below(tag + ".sigma_max", np.max(np.abs(sig[c] - want) / want), TOL_SIGMA)


# ---- 1. the drawn path's channel, passed back as it is ---------------------------------------------------------------------------
def test_drawn_channel_passed_back_gives_the_drawn_paths_bits():
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=4, Nr=16, L=3, T=6, Mr=4)
    kw = dict(seed=77, sweep_idx=2, want_H=True, want_draws=True, with_hbf=True)
    a = build_trials(p, 5, 3, **kw)
    H = a["H"].reshape(3, p.Nr, p.L, p.Nt).permute(0, 1, 3, 2)                           # (3, Nr, Nt, L)
    b = build_trials(p, 5, 3, channel=H, channel_normalize="asis", **kw)
    torch.cuda.synchronize()
    assert set(b) == (set(a) - {"gains", "u_r", "u_t"}) | {"sigma_max"}
    for k in ("H", "Zbar", "subY", "Omega", "B", "A", "indx_S", "tau_Y", "tau_Z", "rho", "noise", "qam_idx", "pilot_sym", "Y_hbf",
              "A_hbf", "B_hbf"):
        assert torch.equal(a[k], b[k]), k
    assert b["sigma_max"].shape == (3, p.L) and b["sigma_max"].dtype == torch.float64
    assert torch.isfinite(b["sigma_max"]).all() and (b["sigma_max"] > 0).all()


# ---- 2. against the oracle, every normalisation ----------------------------------------------------------------------------------
SHAPES = [("cut16x5", dict(Nt=3, Nr=12, L=2, T=5, Mr=3), (16, 5)),                      # ld > n, rows no multiple of anything
          ("rowside", dict(Nt=6, Nr=4, L=2, T=3, Mr=2, rho_rule="max"), (4, 6)),        # Nr < Nt: the Gram on the row side
          ("order1", dict(Nt=1, Nr=8, L=1, T=8, Mr=2), (8, 1)),                          # order-1 Gram
          ("driver", dict(Nt=4, Nr=32, L=4, T=25, Mr=4, Mr_e=32), (32, 4)),             # plot_errorVSsnr_nyuwireless.m:9-24
          ("lds64", dict(Nt=64, Nr=64, L=1, T=1, Mr=8, Mr_e=64, T_prop=64), (64, 64))]  # the LDS limit of the Jacobi


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,kw,src_shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_against_the_oracle(name, kw, src_shape, mode):
    from jstsp19_amd.system_model import build_trials
    p = _sp(snr_db=5.0, **kw)
    src = _c64(make_channel(src_shape[0], src_shape[1], p.L, 21, "paths"))
    hbf = p.T_hbf > 0
    out = build_trials(p, 2, 2, seed=5, sweep_idx=1, want_H=True, want_draws=True, with_hbf=hbf, channel=src,
                       channel_normalize=mode)
    torch.cuda.synchronize()
    N, M, Gr, G2 = p.solver_shape
    assert out["subY"].stride() == (N * M, 1, N) and out["H"].stride() == (p.Nr * p.Nt * p.L, 1, p.Nr)
    assert "gains" not in out and out["sigma_max"].shape == (p.L,)
    for t in range(2):
        _compare("given.%s.%s" % (name, mode), p, out, src, mode, t, hbf)
    _check_sigma("given.%s" % name, p, out, src)
    if mode == "asis":                                                                  # the stored bits are the input bits
        Hm = out["H"][0].cpu().numpy().reshape(p.Nr, p.L, p.Nt).transpose(0, 2, 1)
        np.testing.assert_array_equal(Hm, src[:p.Nr, :p.Nt, :])


# ---- 3. spectra that stress the Jacobi -------------------------------------------------------------------------------------------
P3 = dict(Nt=4, Nr=12, L=3, T=5, Mr=3, snr_db=5.0)
D3 = [(1.0,), (2.0, 2.0, 0.5), (1.0, 1e-3, 1e-6, 0.0)]            # rank 1; the two largest equal; a graded spectrum with a zero


@pytest.mark.parametrize("mode", MODES)
def test_stress_spectra(mode):
    from jstsp19_amd.system_model import build_trials
    p = _sp(**P3)
    src = _c64(make_channel(12, 4, 3, 8, "svd", d=D3))
    out = build_trials(p, 0, 2, seed=2, want_H=True, want_draws=True, with_hbf=True, channel=src, channel_normalize=mode)
    torch.cuda.synchronize()
    for t in range(2):
        _compare("given.svd.%s" % mode, p, out, src, mode, t, True)
    _check_sigma("given.svd", p, out, src)
    # the prescribed values themselves, to what narrowing the entries to complex64 leaves of them
    np.testing.assert_allclose(out["sigma_max"].numpy(), [1.0, 2.0, 1.0], rtol=1e-6)


def test_taps_of_size_2_to_the_40_lose_nothing():
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=4, Nr=12, L=2, T=5, Mr=3, snr_db=5.0)
    src = _c64(make_channel(12, 4, 2, 9, "svd", d=[(1.0, 0.5, 0.25, 0.125), (1.0, 1e-3, 1e-6, 0.0)]))
    big = src.copy()
    big[:, :, 0] *= np.float32(2.0 ** 40)
    big[:, :, 1] *= np.float32(2.0 ** -40)
    assert np.array_equal(big[:, :, 0].astype(complex) * 2.0 ** -40, src[:, :, 0].astype(complex))        # (exact scalings)
    assert np.array_equal(big[:, :, 1].astype(complex) * 2.0 ** 40, src[:, :, 1].astype(complex))
    kw = dict(seed=4, want_H=True, want_draws=True, with_hbf=True)
    a = build_trials(p, 0, 2, channel=src, channel_normalize="unit", **kw)
    b = build_trials(p, 0, 2, channel=big, channel_normalize="unit", **kw)
    torch.cuda.synchronize()
    want = a["sigma_max"].numpy() * np.array([2.0 ** 40, 2.0 ** -40])
    np.testing.assert_array_equal(b["sigma_max"].numpy(), want)
    assert torch.equal(a["H"], b["H"])
    _check_sigma("given.pow2", p, b, big)
    for t in range(2):
        _compare("given.pow2.unit", p, b, big, "unit", t, True)


# ---- 4. shared and per-trial channels --------------------------------------------------------------------------------------------
def test_shared_and_per_trial_channels():
    from jstsp19_amd.system_model import build_trials
    p = _sp(Nt=3, Nr=12, L=2, T=5, Mr=3, snr_db=0.0)
    src = _c64(make_channel(16, 5, 2, 3, "paths"))
    kw = dict(seed=6, sweep_idx=1, want_H=True, want_draws=True, with_hbf=True, channel_normalize="reference")
    a = build_trials(p, 4, 3, channel=src, **kw)
    b = build_trials(p, 4, 3, channel=np.stack([src] * 3), **kw)
    torch.cuda.synchronize()
    assert a["sigma_max"].shape == (2,) and b["sigma_max"].shape == (3, 2)
    for k in a:
        if k == "sigma_max":
            assert all(torch.equal(a[k], b[k][t]) for t in range(3))
        else:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["Zbar"][0], a["Zbar"][1]) and torch.equal(a["Zbar"][0], a["Zbar"][2])
    assert torch.equal(a["H"][0], a["H"][2]) and not torch.equal(a["subY"][0], a["subY"][1])
    # per-trial channels: trial 1 of a batch of 3 is trial0 + 1 in a batch of 1
    per = _c64(np.stack([make_channel(16, 5, 2, 30 + t, "paths") for t in range(3)]))
    c = {k: v.clone() for k, v in build_trials(p, 4, 3, channel=per, **kw).items()}
    d = build_trials(p, 5, 1, channel=per[1:2], **kw)
    torch.cuda.synchronize()
    for k in d:
        if k in ("A", "A_hbf"):
            assert torch.equal(c[k], d[k]), k
        else:
            assert torch.equal(c[k][1:2], d[k]), k
    assert not torch.equal(c["Zbar"][0], c["Zbar"][1])
    # a CUDA tensor already in the device layout is used where it is
    from jstsp19_amd.system_model import _channel_on_device
    dev = _channel_on_device(per, a["H"].device)
    assert dev.stride() == (16 * 5 * 2, 1, 16, 80) and _channel_on_device(dev, dev.device) is dev
    e = build_trials(p, 4, 3, channel=dev, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(c[k], e[k]) for k in c)


# ---- the C ABI by hand: both memspaces, the refusals ------------------------------------------------------------------------------
OUT_KEYS = ("subY", "Omega", "A", "B", "Zbar", "H", "indx_S")
SENTINEL = 7.0


def _flat(src, pad=0):
    """The buffer the C ABI reads: every tap column-major, tap after tap; channels of a per-trial array ``pad`` elements apart."""
    src = np.asarray(src)
    chans = src.reshape((-1,) + src.shape[-3:])
    rows = [np.concatenate([c.reshape(-1, order="F"), np.zeros(pad, src.dtype)]) for c in chans]
    return np.ascontiguousarray(np.concatenate(rows).astype(np.complex64))


def _raw_call(p, batch, src, ld_rows, ld_cols, stride, normalize, memspace, *, want_sigma=True, gains=False, n_sig=None,
              null_src=False, pad=0):
    """jstsp_build_trials_from_channel_c32 through ctypes with seed 13, sweep 1, trial0 2: ``src`` (Nr_src, Nt_src, L) or
    (batch, Nr_src, Nt_src, L), handed over as ``_flat(src, pad)`` in host memory or copied to the device, like the outputs
    (pre-filled with SENTINEL).  Returns (rc, outputs as flat numpy arrays in memory order, sigma_max, message)."""
    from jstsp19_amd import _lib
    ctx = _lib.default_context(0)
    ctx.use_torch_stream()
    N, M, Gr, G2 = p.solver_shape
    sizes = dict(subY=(batch * N * M, np.complex64), Omega=(batch * N * M, np.float32), A=(N * Gr, np.complex64),
                 B=(batch * G2 * M, np.complex64), Zbar=(batch * Gr * G2, np.complex64),
                 H=(batch * p.Nr * p.Nt * p.L, np.complex64), indx_S=(batch * Gr * G2, np.int32))
    if gains:
        sizes["gains"] = (batch * p.L, np.complex64)
    host = {k: np.full(n, SENTINEL, dtype=dt) for k, (n, dt) in sizes.items()}
    flat = _flat(src, pad)
    if memspace == _lib.DEVICE:
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        dsrc = torch.from_numpy(flat).cuda()
        ptr = lambda k: dev[k].data_ptr()
        src_ptr = dsrc.data_ptr()
    else:
        ptr = lambda k: host[k].ctypes.data
        src_ptr = flat.ctypes.data
    tr = _lib.Trials()
    for k in sizes:
        setattr(tr, k, ptr(k))
    hyp = {k: np.full(batch, SENTINEL) for k in ("tau_Y", "tau_Z", "rho")}
    for k, v in hyp.items():
        setattr(tr, k, v.ctypes.data_as(C.POINTER(C.c_double)))
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, 0, 0, 0, 0, p.noise_var, _lib.BF_ZC, _lib.RHO_MIN6, 1.0,
                       _lib.PILOTS_QAM4)
    sig = np.full(n_sig if n_sig is not None else (p.L if stride == 0 else p.L * batch), SENTINEL)
    rc = ctx._lib.jstsp_build_trials_from_channel_c32(
        ctx.handle, C.byref(model), C.c_uint64(13), 1, 2, batch, None if null_src else src_ptr, ld_rows, ld_cols, stride,
        normalize, C.byref(tr), sig.ctypes.data_as(C.POINTER(C.c_double)) if want_sigma else None, memspace)
    torch.cuda.synchronize()
    if memspace == _lib.DEVICE:
        host = {k: v.cpu().numpy() for k, v in dev.items()}
    host.update(hyp)
    msg = ctx._lib.jstsp_last_error().decode() if rc else ""
    return rc, host, sig, msg


def _untouched(o, sig):
    return all(np.all(v == v.dtype.type(SENTINEL)) for v in o.values()) and np.all(sig == SENTINEL)


P5 = dict(Nt=3, Nr=12, L=2, T=5, Mr=3, snr_db=0.0)


def test_both_memspaces_return_the_same_bits():
    from jstsp19_amd import _lib
    p = _sp(**P5)
    per = np.stack([_c64(make_channel(16, 5, 2, 40 + t, "paths")) for t in range(2)])
    for src, stride, pad in ((per[0], 0, 0), (per, 160 + 7, 7)):                       # shared; per trial with a padded stride
        (rh, oh, sh, _), (rd, od, sd, _) = [_raw_call(p, 2, src, 16, 5, stride, _lib.CHAN_REFERENCE, ms, pad=pad)
                                            for ms in (_lib.HOST, _lib.DEVICE)]
        assert rh == 0 and rd == 0
        for k in ("H", "Zbar", "subY", "Omega", "A", "B", "indx_S", "tau_Y", "tau_Z", "rho"):
            np.testing.assert_array_equal(oh[k], od[k], err_msg=k)
        np.testing.assert_array_equal(sh, sd)
        assert not np.any(sh == SENTINEL) and not np.any(oh["H"] == SENTINEL)
    # and the padded per-trial call is the Python wrapper's call on the same channels
    from jstsp19_amd.system_model import build_trials
    w = build_trials(p, 2, 2, seed=13, sweep_idx=1, want_H=True, channel=per, channel_normalize="reference")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(w["H"].transpose(1, 2).contiguous().cpu().numpy().reshape(-1), od["H"])
    np.testing.assert_array_equal(w["sigma_max"].numpy().reshape(-1), sd)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ARG, E_ILLCOND = -1, -2, -3, -4, -6


@pytest.mark.parametrize("bad", [np.nan, np.inf, complex(0.0, -np.inf)])
@pytest.mark.parametrize("mode", [0, 2])
def test_non_finite_entry_in_a_used_block_is_refused(bad, mode):
    from jstsp19_amd import _lib
    p = _sp(**P5)
    per = np.stack([_c64(make_channel(16, 5, 2, 50 + t, "paths")) for t in range(3)])
    per[1, 11, 2, 1] = bad                                 # the last used row and column of tap 1 of the call's second trial
    rc, o, sig, msg = _raw_call(p, 3, per, 16, 5, 160, mode, _lib.DEVICE)
    assert rc == E_ILLCOND and "tap 1" in msg and "trial 3" in msg and "NaN or Inf" in msg          # trial0 = 2
    assert _untouched(o, sig)
    rc, o, sig, msg = _raw_call(p, 1, per[1], 16, 5, 0, mode, _lib.HOST)
    assert rc == E_ILLCOND and "tap 1" in msg and "shared" in msg and _untouched(o, sig)


def test_non_finite_entry_outside_the_used_block_is_ignored():
    from jstsp19_amd import _lib
    p = _sp(**P5)
    src = _c64(make_channel(16, 5, 2, 60, "paths"))
    dirty = src.copy()
    dirty[12:, :, :] = np.nan                              # unused rows
    dirty[:, 3:, 1] = np.inf                               # unused columns
    a = _raw_call(p, 2, src, 16, 5, 0, _lib.CHAN_UNIT, _lib.DEVICE)
    b = _raw_call(p, 2, dirty, 16, 5, 0, _lib.CHAN_UNIT, _lib.DEVICE)
    assert a[0] == 0 and b[0] == 0
    for k in a[1]:
        np.testing.assert_array_equal(a[1][k], b[1][k], err_msg=k)
    np.testing.assert_array_equal(a[2], b[2])


def test_all_zero_tap():
    from jstsp19_amd import _lib
    p = _sp(**P5)
    src = _c64(make_channel(16, 5, 2, 61, "paths"))
    src[:12, :3, 1] = 0                                    # the used block only
    for mode in (_lib.CHAN_REFERENCE, _lib.CHAN_UNIT):
        rc, o, sig, msg = _raw_call(p, 2, src, 16, 5, 0, mode, _lib.DEVICE)
        assert rc == E_ILLCOND and "tap 1" in msg and "zero" in msg and _untouched(o, sig)
    rc, o, sig, _ = _raw_call(p, 2, src, 16, 5, 0, _lib.CHAN_ASIS, _lib.DEVICE)
    assert rc == 0 and sig[1] == 0.0 and sig[0] > 0 and np.all(np.isfinite(o["subY"])) and not np.any(o["H"] == SENTINEL)


def test_bad_arguments():
    from jstsp19_amd import _lib
    p = _sp(**P5)
    src = _c64(make_channel(16, 5, 2, 62, "paths"))
    for kw, args, code, word in ((dict(), (11, 5, 0, 0), E_SHAPE, "smaller"), (dict(), (16, 2, 0, 0), E_SHAPE, "smaller"),
                                 (dict(), (16, 5, 159, 0), E_SHAPE, "strideH"), (dict(), (16, 5, -160, 0), E_SHAPE, "strideH"),
                                 (dict(), (16, 5, 0, 7), E_ARG, "normalize"), (dict(), (16, 5, 0, -1), E_ARG, "normalize"),
                                 (dict(gains=True), (16, 5, 0, 0), E_ARG, "gains"), (dict(null_src=True), (16, 5, 0, 0), E_NULL, "Hsrc")):
        rc, o, sig, msg = _raw_call(p, 1, src, *args, _lib.DEVICE, n_sig=4, **kw)
        assert rc == code and word in msg, (args, rc, msg)
        assert _untouched(o, sig)


def test_order_above_64_needs_no_norm_only_as_is():
    from jstsp19_amd import _lib
    p = _sp(Nt=65, Nr=65, L=1, T=1, Mr=2, T_prop=4)
    src = _c64(make_channel(65, 65, 1, 63, "paths"))
    rc, o, sig, msg = _raw_call(p, 1, src, 65, 65, 0, _lib.CHAN_UNIT, _lib.DEVICE)
    assert rc == E_UNSUPPORTED and "64" in msg and _untouched(o, sig)
    rc, o, sig, msg = _raw_call(p, 1, src, 65, 65, 0, _lib.CHAN_ASIS, _lib.DEVICE)                 # sigma_max asked for
    assert rc == E_UNSUPPORTED and _untouched(o, sig)
    rc, o, sig, _ = _raw_call(p, 1, src, 65, 65, 0, _lib.CHAN_ASIS, _lib.DEVICE, want_sigma=False)
    assert rc == 0 and np.all(sig == SENTINEL)
    np.testing.assert_array_equal(o["H"], src.reshape(-1, order="F"))
    src[64, 64, 0] = np.nan                                                                        # the check has no such limit
    rc, o, sig, msg = _raw_call(p, 1, src, 65, 65, 0, _lib.CHAN_ASIS, _lib.DEVICE, want_sigma=False)
    assert rc == E_ILLCOND and _untouched(o, sig)
    from jstsp19_amd.system_model import build_trials
    src[64, 64, 0] = 1.0
    w = build_trials(p, 0, 1, channel=src, channel_normalize="asis", want_H=True)
    assert "sigma_max" not in w


# ---- 7. the solvers take what it builds ------------------------------------------------------------------------------------------
def test_solver_on_built_inputs_matches_the_oracle_solver():
    import jstsp19_amd as J
    from jstsp19_amd.system_model import build_trials
    from oracle import solvers as osol
    p = _sp(Nt=4, Nr=16, L=3, T=6, Mr=4, snr_db=10.0)
    src = _c64(make_channel(16, 4, 3, 70, "paths"))
    # "asis": these taps have norm 5..8, and :65-66 as written would leave 1/norm of them, below the noise - S = 0 on both sides
    inp = build_trials(p, 0, 2, seed=8, channel=src, channel_normalize="asis")
    S, Y, _ = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], 20, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(),
                                   inp["rho"].numpy(), "approximate", want_ce=False)
    torch.cuda.synchronize()
    for t in range(2):
        ref = osol.proposed_algorithm(inp["subY"][t].cpu().numpy(), inp["Omega"][t].cpu().numpy(), inp["A"].cpu().numpy(),
                                      inp["B"][t].cpu().numpy(), 20, float(inp["tau_Y"][t]), float(inp["tau_Z"][t]),
                                      float(inp["rho"][t]), "approximate", want_ce=False)
        assert np.count_nonzero(ref[0]) > 20                                               # (a comparison of something)
        check_below("given.solve.S", rel_err(S[t].cpu().numpy(), ref[0]), TOL_S)
        check_below("given.solve.Y", rel_err(Y[t].cpu().numpy(), ref[1]), TOL_S)          # conftest: TOL_S bounds S and Y


# ---- 8. the sweep ----------------------------------------------------------------------------------------------------------------
def test_the_sweep_takes_the_channel_and_nothing_else_changes():
    from jstsp19_amd import montecarlo as mc
    from jstsp19_amd.system_model import build_trials
    pts = mc.driver("errorVSsnr_nyuwireless")["points"][::5]
    # taps of norm 0.26..0.37: "reference" (:65-66 as written) leaves 1/norm of them, 2.7..3.9 - above the noise, so that the
    # columns are not the cap (taps of norm > 1 end below it and every estimator returns 1)
    H = _c64(make_channel(32, 4, 4, 80, "paths") / 32)
    samples = []
    kw = dict(Imax=20, numOfnz=250, baselines=True, batch=4)
    out = mc.run_points(pts, 4, channel=H, samples=samples, **kw)
    assert tuple(out.shape) == (3, 5) and len(samples) == 3 and all(tuple(s.shape) == (4, 5) for s in samples)
    for col in range(5):
        v = out[:, col]
        if col == 3 and torch.isnan(v).all():             # VAMP: NaN where run_points documents it
            continue
        assert torch.isfinite(v).all() and float(v.min()) >= 0.0 and float(v.max()) <= 1.0, (col, v)
    assert float(out[1:, :2].max()) < 1.0 and all(float(s[:, 0].min()) < 1.0 for s in samples[1:])      # (not the cap)
    solve = mc._hip_solvers(torch.device("cuda", torch.cuda.current_device()))
    for k, p in enumerate(pts):
        inp = build_trials(p, 0, 4, sweep_idx=k, channel=H, with_hbf=True)
        e, ea = solve(inp, 20, p.noise_var)
        e = e.double().cpu()
        assert torch.equal(samples[k][:, 0], e)
        assert float(out[k, 0]) == float(e.sum()) / 4
    # the channel enters in no other way: 3 H under "unit" is H / norm under "asis"
    unit = cut_and_scale(pts[0], H.astype(complex), "unit")[0]
    a = mc.run_points(pts, 4, channel=_c64(3 * H.astype(complex)), channel_normalize="unit", **kw)
    inp3 = build_trials(pts[0], 0, 1, channel=_c64(3 * H.astype(complex)), channel_normalize="unit", want_H=True)
    Hn = inp3["H"][0].reshape(32, 4, 4).permute(0, 2, 1).contiguous().cpu().numpy()      # the normalised channel, as built
    check_below("given.sweep.unit_H", rel_err(Hn, unit), 2e-6)
    b = mc.run_points(pts, 4, channel=Hn, channel_normalize="asis", **kw)
    assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
