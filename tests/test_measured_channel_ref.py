"""The supplied-channel path without a GPU: the float64 helper of its GPU tests is tied to the oracle, the normalisation rule of
plot_errorVSsnr_nyuwireless.m:65-66, the channel loader, the driver preset and the Python-side refusals of ``build_trials``."""
import numpy as np
import pytest

from measured_channel_ref import cut_and_scale, make_channel, oracle_params, reference_inputs


def _p(**kw):
    from jstsp19_amd.system_model import SweepParams
    return SweepParams(**kw)


@pytest.mark.parametrize("kw", [dict(Nt=4, Nr=16, L=3, T=6, Mr=4, snr_db=5.0),
                                dict(Nt=2, Nr=12, L=2, T=7, Mr=3, Mr_e=9, Gr=16, Gt=4, clusters=3, rays=2, snr_db=10.0),
                                dict(Nt=6, Nr=32, L=4, T=10, Mr=4, snr_db=15.0, beamformer="fft", rho_rule="max")])
def test_helper_equals_the_oracle_on_the_oracles_own_channel(kw):
    """normalize = "asis" on H of wideband_mmwave_channel: reference_inputs is training_inputs_errorVSsnr on the same draws."""
    from oracle import system_model as osm
    p = _p(**kw)
    params = oracle_params(p)
    draws = osm.draw_trial(np.random.default_rng(3), params)
    want = osm.training_inputs_errorVSsnr(params, draws)
    H = osm.wideband_mmwave_channel(p.L, p.Nr, p.Nt, p.clusters, p.rays, p.Gr, p.Gt, draws["gains"], draws["u_r"], draws["u_t"])[0]
    got = reference_inputs(p, H, "asis", draws)
    assert set(want) <= set(got)
    for k, w in want.items():
        w = np.asarray(w)
        scale = float(np.max(np.abs(w))) if w.size else 0.0
        assert np.allclose(got[k], w, rtol=1e-13, atol=1e-13 * scale), k
    np.testing.assert_array_equal(got["indx_S"], want["indx_S"])


@pytest.mark.parametrize("kind", ["paths", "svd"])
def test_normalisation_rule(kind):
    """:65-66 as written leaves a tap of spectral norm 1/s; "unit" leaves 1; "asis" the cut block itself."""
    p = _p(Nt=3, Nr=12, L=2, T=5, Mr=3)
    src = make_channel(16, 5, 2, 11, kind)
    cut = src[:12, :3, :]
    s = np.array([np.linalg.norm(cut[:, :, l], 2) for l in range(2)])
    for mode, want in (("reference", 1 / s), ("unit", np.ones(2)), ("asis", s)):
        H, sig = cut_and_scale(p, src, mode)
        np.testing.assert_allclose(sig, s, rtol=1e-14)
        got = np.array([np.linalg.norm(H[:, :, l], 2) for l in range(2)])
        np.testing.assert_allclose(got, want, rtol=1e-13)
    np.testing.assert_array_equal(cut_and_scale(p, src, "asis")[0], cut)


def test_make_channel_svd_has_the_prescribed_norm():
    H = make_channel(12, 4, 3, 5, "svd", d=[(1.0,), (2.0, 2.0, 0.5), (1.0, 1e-3, 1e-6, 0.0)])
    for l, s in enumerate((1.0, 2.0, 1.0)):
        np.testing.assert_allclose(np.linalg.norm(H[:, :, l], 2), s, rtol=1e-13)
    assert np.linalg.matrix_rank(H[:, :, 0]) == 1


def test_load_channel_round_trips(tmp_path):
    from jstsp19_amd.montecarlo import load_channel
    H = make_channel(6, 3, 2, 1, "paths")
    np.save(tmp_path / "h.npy", H)
    np.testing.assert_array_equal(load_channel(str(tmp_path / "h.npy")), H)
    for key in ("Hf", "H"):
        np.savez(tmp_path / ("%s.npz" % key), **{key: H})
        np.testing.assert_array_equal(load_channel(str(tmp_path / ("%s.npz" % key))), H)
    np.savez(tmp_path / "other.npz", X=H)
    with pytest.raises(ValueError, match="Hf"):
        load_channel(str(tmp_path / "other.npz"))
    with pytest.raises(ValueError, match="npy"):
        load_channel(str(tmp_path / "h.txt"))
    (tmp_path / "v73.mat").write_bytes(b"MATLAB 7.3 MAT-file, Platform: GLNXA64".ljust(128) + b"\0" * 384 + b"\x89HDF\r\n\x1a\n")
    with pytest.raises(ValueError, match="v7.3"):
        load_channel(str(tmp_path / "v73.mat"))


def test_load_channel_reads_the_cell_array_of_a_mat_file(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from jstsp19_amd.montecarlo import load_channel
    H = make_channel(6, 3, 2, 2, "paths")
    cells = np.empty((1, 2), dtype=object)
    for l in range(2):
        cells[0, l] = H[:, :, l]
    sio.savemat(str(tmp_path / "nywireless_like.mat"), {"Hf": cells})
    np.testing.assert_array_equal(load_channel(str(tmp_path / "nywireless_like.mat")), H)


def test_driver_preset():
    """plot_errorVSsnr_nyuwireless.m:9-26."""
    from jstsp19_amd.montecarlo import driver
    d = driver("errorVSsnr_nyuwireless")
    assert d["needs_channel"] is True and not driver("errorVSsnr").get("needs_channel")
    assert (d["Imax"], d["numOfnz"], d["n_trials"], d["metric"], d["axis"]) == (100, 250, 50, "nmse", "snr_db")
    assert d["values"] == list(range(-15, 16, 3)) and len(d["points"]) == 11
    for v, p in zip(d["values"], d["points"]):
        assert (p.Nt, p.Nr, p.L, p.T, p.Mr, p.Mr_e, p.Gr, p.Gt) == (4, 32, 4, 25, 4, 32, 32, 4)
        assert (p.beamformer, p.rho_rule, p.rho_scale, p.T_prop, p.T_hbf, p.snr_db) == ("ZC", "min", 1.0, 100, 12, float(v))


def test_run_driver_without_a_channel_says_where_it_goes():
    from jstsp19_amd.montecarlo import run_driver, run_points
    with pytest.raises(ValueError, match="channel="):
        run_driver("errorVSsnr_nyuwireless", 2)
    H = make_channel(32, 4, 4, 0, "paths")
    with pytest.raises(ValueError, match="builder"):
        run_points([_p(Nt=4, Nr=32, L=4, T=25, Mr=4)], 2, channel=H, builder=lambda *a: None, device="cpu")


def test_build_trials_refuses_a_bad_channel_before_the_library_is_loaded(monkeypatch):
    from jstsp19_amd import _lib
    from jstsp19_amd.system_model import build_trials

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(_lib, "default_context", no_library)
    p = _p(Nt=3, Nr=12, L=2, T=5, Mr=3)
    good = make_channel(16, 5, 2, 0, "paths")
    with pytest.raises(ValueError, match="delay taps"):
        build_trials(p, 0, 2, channel=make_channel(16, 5, 3, 0, "paths"))
    with pytest.raises(ValueError, match="smaller"):
        build_trials(p, 0, 2, channel=good[:11])
    with pytest.raises(ValueError, match="smaller"):
        build_trials(p, 0, 2, channel=good[:, :2])
    with pytest.raises(TypeError, match="complex"):
        build_trials(p, 0, 2, channel=good.real)
    with pytest.raises(ValueError, match="per trial"):
        build_trials(p, 0, 2, channel=np.stack([good] * 3))
    with pytest.raises(ValueError, match="Nr_src"):
        build_trials(p, 0, 2, channel=good[:, :, 0])
    with pytest.raises(ValueError, match="channel_normalize"):
        build_trials(p, 0, 2, channel=good, channel_normalize="norm")
