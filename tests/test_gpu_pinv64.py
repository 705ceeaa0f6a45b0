"""jstsp_pinv_f64 / jstsp_ls_f64 (csrc/pinv64.hip) on the GPU against problems with a known pseudo-inverse
(tests/pinv64_problems.py; tests/test_pinv64_problems.py shows on the CPU that a Gram route fails these bounds).

The bound is measured against numpy, not fixed: with d_ref = ||numpy.linalg.pinv(A) - P_exact||_2 / ||P_exact||_2 the device
must give ||P_dev - P_exact||_2 / ||P_exact||_2 <= 8 * max(d_ref, cond * 2^-53); rcond against s_r / s_1 of the construction
with the same bound, relative; rank exactly.  No case is skipped.
"""
import numpy as np
import pytest
import torch

import pinv64_problems as Q
from conftest import check_below

import jstsp19_amd as J

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype.itemsize % 8 == 0 else np.uint32)


def differing(a, b):
    """number of entries of a and b whose bits differ"""
    a, b = bits(a), bits(b)
    return float(a.size + b.size) if a.shape != b.shape else float(np.count_nonzero(a != b))


def on_device(x):
    return J.colmajor(torch.from_numpy(np.ascontiguousarray(x)).to(DEV))


@pytest.mark.parametrize("case", Q.CASES, ids=Q.case_id)
def test_pinv_is_within_eight_times_numpy_of_the_exact_pseudo_inverse(case):
    rows, cols, cond, rank = case
    A, P, s = Q.build(case)
    bound = Q.device_bound(case)
    name = Q.case_id(case)
    Ph, rch, rkh = J.pinv_f64(A, info=True)                                   # host memspace
    Pd, rcd, rkd = J.pinv_f64(on_device(A), info=True)                        # device memspace
    assert Ph.shape == (cols, rows) and Ph.dtype == np.complex128 and Pd.dtype == torch.complex128
    err = Q.rel2(np.asarray(Ph), P)
    print("%s: device %.3g, numpy %.3g, bound %.3g (device / (cond 2^-53) = %.3g)" % (name, err, Q.numpy_error(case), bound, err / (cond * Q.EPS53)))
    check_below("pinv64/error_over_bound", err / bound, 1.0)
    check_below("pinv64/device_memspace_bits_differ", differing(Pd, Ph), 0.5)
    check_below("pinv64/device_memspace_bits_differ", differing(rcd, rch) + differing(rkd, rkh), 0.5)
    check_below("pinv64/rcond_error_over_bound", abs(float(rch) - s[-1] / s[0]) / (s[-1] / s[0]) / bound, 1.0)
    check_below("pinv64/rank_mismatch", abs(int(rkh) - len(s)), 0.5)


def test_complex64_input_is_widened_exactly_and_a_repeated_call_returns_the_same_bits():
    for case in ((140, 16, 1e5, None), (16, 140, 1e5, None), (512, 640, 1e2, 300)):
        A = Q.build(case)[0].astype(np.complex64)
        P32, P64 = J.pinv_f64(A), J.pinv_f64(A.astype(np.complex128))
        check_below("pinv64/complex64_bits_differ", differing(P32, P64), 0.5)
        check_below("pinv64/repeat_bits_differ", differing(J.pinv_f64(A), P32), 0.5)
        Pd = J.pinv_f64(on_device(A))
        check_below("pinv64/complex64_bits_differ", differing(Pd, P64), 0.5)


def test_zero_matrix_and_repeated_column():
    P, rc, rk = J.pinv_f64(np.zeros((40, 24), dtype=np.complex128), info=True)
    check_below("pinv64/zero_matrix_nonzeros", float(np.count_nonzero(np.asarray(P))) + abs(float(rc)) + abs(int(rk)), 0.5)
    A = Q.repeated_column()
    P, rc, rk = J.pinv_f64(A, info=True)
    sv = np.linalg.svd(A, compute_uv=False)
    cond_kept = sv[0] / sv[A.shape[1] - 2]
    check_below("pinv64/rank_mismatch", abs(int(rk) - (A.shape[1] - 1)), 0.5)
    ref = Q.penrose(A, Q.numpy_pinv(A))
    got = Q.penrose(A, np.asarray(P))
    for i in range(4):
        print("Penrose %d: device %.3g, numpy %.3g" % (i + 1, got[i], ref[i]))
        check_below("pinv64/penrose_%d_over_bound" % (i + 1), got[i] / (8.0 * max(ref[i], cond_kept * Q.EPS53)), 1.0)


def test_a_nan_stays_in_its_own_matrix_and_batch_mates_equal_their_stand_alone_calls():
    Ab, Pb, conds, ranks = Q.batch_of_five()
    P, rc, rk = J.pinv_f64(Ab, info=True)
    for t in range(5):
        err = Q.rel2(np.asarray(P[t]), Pb[t])
        bound = 8.0 * max(Q.rel2(Q.numpy_pinv(Ab[t]), Pb[t]), conds[t] * Q.EPS53)
        print("batch matrix %d: %.3g (bound %.3g)" % (t, err, bound))
        check_below("pinv64/error_over_bound", err / bound, 1.0)
        check_below("pinv64/rank_mismatch", abs(int(rk[t]) - ranks[t]), 0.5)
        check_below("pinv64/batch_vs_alone_bits_differ", differing(np.asarray(P[t]), J.pinv_f64(Ab[t])), 0.5)
    bad = Ab.copy()
    bad[2, 3, 4] = np.nan
    Pn, rcn, rkn = J.pinv_f64(bad, info=True)
    assert np.isnan(np.asarray(Pn[2])).all() and np.isnan(rcn[2]) and rkn[2] == 0
    for t in (0, 1, 3, 4):
        check_below("pinv64/batch_vs_alone_bits_differ", differing(np.asarray(Pn[t]), np.asarray(P[t])), 0.5)
        check_below("pinv64/batch_vs_alone_bits_differ", differing(rcn[t], rc[t]) + differing(rkn[t], rk[t]), 0.5)
    bad[2, 3, 4] = np.inf
    assert np.isnan(np.asarray(J.pinv_f64(bad)[2])).all()
    check_below("pinv64/repeat_bits_differ", differing(J.pinv_f64(Ab), P), 0.5)


@pytest.mark.parametrize("shape", [(24, 40, 16, 20, 3, 1e3, 1e5), (64, 512, 64, 128, 2, 1e5, 1e7)], ids=lambda s: "N%d-M%d" % s[:2])
def test_ls_estimate_against_numpy(shape):
    N, M, Gr, G2, batch, cA, cB = shape
    rng = np.random.default_rng([20190913, N, M, Gr, G2])
    fa = [Q.factor(rng, N, Gr, cA) for _ in range(batch)]
    fb = [Q.factor(rng, G2, M, cB) for _ in range(batch)]
    Y = (rng.standard_normal((batch, N, M)) + 1j * rng.standard_normal((batch, N, M))) / np.sqrt(2)
    A, B = np.stack([f[0] for f in fa]), np.stack([f[0] for f in fb])
    S, rc = J.ls_estimate_f64(Y, A, B, info=True)                                             # per-trial factors
    for t in range(batch):
        exact = fa[t][1] @ Y[t] @ fb[t][1]
        ref = Q.numpy_pinv(A[t]) @ Y[t] @ Q.numpy_pinv(B[t])
        scale = np.linalg.norm(ref, 2)
        d_ref = np.linalg.norm(ref - exact, 2) / scale
        err = np.linalg.norm(np.asarray(S[t]) - exact, 2) / scale
        bound = 8.0 * max(d_ref, (cA + cB) * Q.EPS53)
        print("ls trial %d: device %.3g, numpy %.3g, bound %.3g" % (t, err, d_ref, bound))
        check_below("ls64/error_over_bound", err / bound, 1.0)
    check_below("ls64/rcond_error_over_bound", max(abs(rc[0] * cA - 1.0) / (8 * cA * Q.EPS53), abs(rc[1] * cB - 1.0) / (8 * cB * Q.EPS53)), 1.0)
    # shared factors: the same bits as per-trial copies of them, host and device
    A0, B0 = A[0], B[0]
    Ss = J.ls_estimate_f64(Y, A0, B0)
    Sc = J.ls_estimate_f64(Y, np.stack([A0] * batch), np.stack([B0] * batch))
    check_below("ls64/shared_vs_copies_bits_differ", differing(Ss, Sc), 0.5)
    Sd = J.ls_estimate_f64(on_device(Y), on_device(A0), on_device(B0))
    check_below("ls64/device_memspace_bits_differ", differing(Sd, Ss), 0.5)
    check_below("ls64/repeat_bits_differ", differing(J.ls_estimate_f64(Y, A0, B0), Ss), 0.5)
    S32 = J.ls_estimate_f64(Y.astype(np.complex64), A0.astype(np.complex64), B0.astype(np.complex64))
    S64 = J.ls_estimate_f64(Y.astype(np.complex64).astype(np.complex128), A0.astype(np.complex64).astype(np.complex128),
                            B0.astype(np.complex64).astype(np.complex128))
    check_below("ls64/complex64_bits_differ", differing(S32, S64), 0.5)


def test_agreement_with_the_fp32_storing_entry_where_it_works():
    case = (64, 64, 1e2, None)
    A = Q.build(case)[0].astype(np.complex64)
    P32 = np.asarray(J.pinv(A))
    P64 = np.asarray(J.pinv_f64(A)).astype(np.complex64)
    check_below("pinv64/vs_pinv_c32", Q.rel2(P64, P32), 13 * 6e-8 * 1e2)


def test_limits_are_refused():
    for rows, cols in ((513, 600), (16, 8200)):
        with pytest.raises(J.JstspError) as e:
            J.pinv_f64(np.zeros((rows, cols), dtype=np.complex128))
        assert e.value.code == -3
    with pytest.raises(J.JstspError) as e:
        J.ls_estimate_f64(np.zeros((16, 8200), complex), np.zeros((16, 8), complex), np.zeros((8, 8200), complex))
    assert e.value.code == -3


def _same(a, b):
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    return float(np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def test_ls_precision_f64_gives_numbers_where_the_default_cannot_at_baseline_configs1():
    """The case the feature exists for: the conventional-HBF inputs of the sweep runner at the BASELINE configs[1] shape
    (B_hbf 512 x 512 per trial, from the library's own generator)."""
    from jstsp19_amd import montecarlo as mc
    from jstsp19_amd.system_model import SweepParams, build_trials
    from oracle import solvers as O
    p = SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=5.0)
    inp = build_trials(p, 0, 4, seed=20190913, sweep_idx=0, device=torch.device(DEV, 0), with_hbf=True)
    assert inp["B_hbf"].shape[1] == 512

    def default(i):
        try:
            return mc._hip_baselines(i, 100)
        except J.JstspError as e:
            if e.code != -6:
                raise
            return None

    d1 = default(inp)
    if d1 is not None and not torch.isnan(d1["ls"]).any():
        # the default copes with this seed's B_hbf: the stand-in the fp32 Gram route cannot invert
        rng = np.random.default_rng(7)
        Bs = Q.factor(rng, 512, inp["B_hbf"].shape[2], 1e7)[0].astype(np.complex64)
        inp = dict(inp)
        inp["B_hbf"] = on_device(np.stack([Bs] * 4))
        d1 = default(inp)
    assert d1 is None or torch.isnan(d1["ls"]).all(), "the default path was expected to have no LS number here"
    f = mc._hip_baselines(inp, 100, ls_precision="f64")
    assert torch.isfinite(f["ls"]).all() and torch.isfinite(f["omp_mmv"]).all()
    A, B, Y = (inp[k].cpu().numpy().astype(np.complex128) for k in ("A_hbf", "B_hbf", "Y_hbf"))
    zb = inp["Zbar"].cpu().numpy().astype(np.complex128)
    for t in range(4):
        At = A if A.ndim == 2 else A[t]
        ref = O.nmse_capped(np.linalg.pinv(At) @ Y[t] @ np.linalg.pinv(B[t]), zb[t])
        print("trial %d: LS NMSE device %.12g, numpy %.12g, cond(B_hbf) %.3g" % (t, float(f["ls"][t]), ref, np.linalg.cond(B[t])))
        check_below("ls64/baseline_configs1_dNMSE", abs(float(f["ls"][t]) - ref), 1e-9)
    # the default call is what it was: the same values as the unchanged default path, before and after the float64 call
    d2 = default(inp)
    assert (d1 is None) == (d2 is None)
    if d1 is not None:
        for k in d1:
            check_below("ls64/default_path_changed", _same(d1[k], d2[k]), 0.5)
        S_ls = J.ls_estimate(inp["Y_hbf"], inp["A_hbf"], inp["B_hbf"])
        rcond, _ = J.default_context(0).last_conditioning()
        direct = J.nmse_spectral(S_ls, J.colmajor(inp["Zbar"].to(torch.complex64)))
        if rcond * rcond < 1e-6:
            direct = torch.full_like(direct, float("nan"))
        check_below("ls64/default_path_changed", _same(d1["ls"], direct), 0.5)
