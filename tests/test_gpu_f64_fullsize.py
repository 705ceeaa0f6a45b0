"""jstsp_proposed_algorithm_f64 at BASELINE configs[1] (N=64, M=4096, Gr=64, G2=512, Imax=100) against the float64 host port's
results in tests/golden/fullsize_port_heldout2.npz: the trials are rebuilt the way oracle/fullsize_fixture.py: solve_group does
(fingerprint check included) and solved with the hyper-parameters the fixture records.  32 trials of sweep_proposed at each of
-15, 0 and 12 dB and 16 of sweep_angles at 0 dB.

Bounds: |dNMSE| <= 1e-9 per trial - what tests/test_cpu_port.py asks of a second float64 restatement, three orders under the
fp32 path's 1e-6; convergence_error 1e-6 relative on the rows that have it (the fixture stores it as float32: that is its
storage, 6e-8, not this arithmetic).  Measured on MI355X (profiles/f64_measured_tolerances.json): max |dNMSE| 1.04e-13 over the 112 trials,
convergence_error 6.0e-8."""
import numpy as np
import pytest

from conftest import check_below, ce_rel  # noqa: E402

pytestmark = pytest.mark.gpu

IMAX = 100


def _solve_rows(fx, group, rows, angles):
    """(nmse, ce) of the float64 device solve for consecutive fixture rows of one sweep point"""
    import torch
    import jstsp19_amd as J
    from jstsp19_amd.system_model import SweepParams, build_trials
    from oracle import solvers as O
    sidx, trial, snr, fp = (fx[group + "/" + k] for k in ("sweep_idx", "trial", "snr_db", "fingerprint"))
    r = np.asarray(rows)
    assert np.all(np.diff(trial[r]) == 1) and len(set(sidx[r])) == 1 and len(set(snr[r])) == 1
    p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=float(snr[r[0]]))
    seed = int(fx[group + "/seed"][r[0]])
    inp = build_trials(p, int(trial[r[0]]), len(r), seed=seed, sweep_idx=int(sidx[r[0]]))
    f = torch.stack([inp["subY"].abs().double().sum((1, 2)), inp["B"].abs().double().sum((1, 2)),
                     inp["Omega"].double().sum((1, 2))], 1).cpu().numpy()
    np.testing.assert_allclose(f, fp[r][:, :3], rtol=1e-9, err_msg="the generator no longer reproduces the fixture's inputs")
    np.testing.assert_allclose(np.stack([inp[k].numpy() for k in ("tau_Y", "tau_Z", "rho")], 1), fp[r][:, 3:], rtol=2e-6)
    hyp = [np.ascontiguousarray(fp[r][:, 3 + k]) for k in range(3)]
    S, _, ce = J.proposed_algorithm_f64(inp["subY"], inp["Omega"], inp["A"], inp["B"], IMAX, *hyp, "approximate",
                                        indx_S=inp["indx_S"] if angles else None, want_ce=True)
    torch.cuda.synchronize()
    assert S.dtype == torch.complex128
    Sh = S.cpu().numpy()
    zb = inp["Zbar"].cpu().numpy().astype(np.complex128)
    return np.array([O.nmse_capped(Sh[t], zb[t]) for t in range(len(r))]), ce.cpu().numpy()


@pytest.mark.parametrize("group,snr_db,count", [("sweep_proposed", -15.0, 32), ("sweep_proposed", 0.0, 32), ("sweep_proposed", 12.0, 32),
                                                ("sweep_angles", 0.0, 16)])
def test_heldout2_trials_against_the_float64_port(group, snr_db, count):
    from oracle.fullsize_fixture import fixture
    fx = fixture("fullsize_port_heldout2")
    rows = np.nonzero(fx[group + "/snr_db"] == snr_db)[0][:count]
    assert len(rows) == count
    nmse, ce = _solve_rows(fx, group, rows, angles=group == "sweep_angles")
    ref = fx[group + "/nmse_port"][rows]
    d = np.abs(nmse - ref)
    print("f64 fullsize %s %+g dB: max |dNMSE| = %.3e (nmse %.4f .. %.4f)" % (group, snr_db, d.max(), ref.min(), ref.max()))
    for t in range(count):
        check_below("f64.fullsize.nmse", d[t], 1e-9)
    ce_rows = fx[group + "/ce_rows"]
    have = 0
    for t, row in enumerate(rows):
        k = np.nonzero(ce_rows == row)[0]
        if len(k):
            have += 1
            check_below("f64.fullsize.ce", ce_rel(ce[t], fx[group + "/ce_port"][k[0]].astype(np.float64)), 1e-6)
    assert have > 0
