"""tests/golden/cfg5_fullframe_port.npz is what tests/test_gpu_config5_imax100.py takes as the float64 truth at BASELINE configs[4]'s
full frame and Imax = 100: check, without a GPU, that it is whole and self-consistent."""
import numpy as np

from conftest import load_golden

N, M, GR, G2, IMAX = 64, 65536, 64, 4096, 100


def test_cfg5_fullframe_fixture_is_self_consistent():
    fx = load_golden("cfg5_fullframe_port")
    assert int(fx["imax"]) == IMAX and int(fx["seed"]) == 20190913 and int(fx["sweep_idx"]) == 0 and float(fx["snr_db"]) == 5.0
    fp = fx["fingerprint"]
    assert fp.shape == (32, 7) and np.all(np.isfinite(fp)) and np.all(fp[:, [0, 1, 2, 6]] > 0) and np.all(fp[:, 3:6] > 0)
    assert np.all(fp[:, 1] == fp[0, 1])                                  # one pilot set for the batch
    head = 10 + 5 * IMAX
    for g in ("angles", "proposed"):
        t = fx[g + "/trial"]
        n = len(t)
        assert n >= 1 and np.all(np.diff(t) > 0) and t.min() >= 0 and t.max() < 32
        nm, ce = fx[g + "/nmse_port"], fx[g + "/ce_port"]
        assert nm.shape == (n,) and np.all((nm > 0) & (nm <= 1))
        assert ce.shape == (n, IMAX, 3) and ce.dtype == np.float32
        assert np.all(np.isinf(ce[:, 0, 2])) and np.all(np.isfinite(ce[:, 1:, :])) and np.all(np.isfinite(ce[:, :, :2]))
        assert np.all(ce[:, 1:, :] >= 0)
    ix, Sv = fx["angles/indx_S_head"], fx["angles/S_head"]
    assert ix.shape == (len(fx["angles/trial"]), head) and Sv.shape == ix.shape and Sv.dtype == np.complex128
    for i in range(len(ix)):
        assert len(np.unique(ix[i])) == head and ix[i].min() >= 1 and ix[i].max() <= GR * G2      # positions inside indx_S(1:510)
        assert np.all(np.isfinite(Sv[i])) and np.count_nonzero(Sv[i]) > 0
    idx, val = fx["proposed/S_idx"], fx["proposed/S_val"]
    nnz, amax = fx["proposed/S_nnz"], fx["proposed/S_absmax"]
    for i in range(len(idx)):
        k = idx[i] >= 0
        stored = idx[i][k]
        assert len(stored) == min(nnz[i], 16384) and np.all(idx[i][len(stored):] == -1)
        assert len(np.unique(stored)) == len(stored) and stored.max() < GR * G2
        assert np.all(np.isfinite(val[i][k])) and np.all(val[i][k] != 0) and np.all(val[i][~k] == 0)
        assert np.max(np.abs(val[i][k])) == amax[i]                     # the largest entry is among those kept
