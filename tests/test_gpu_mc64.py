"""Matrix completion in float64, jstsp_mc_svt_f64 / jstsp_mc_admm_f64 (csrc/mc64.hip), against oracle/solvers.py mc_svt / mc_admm.

Inputs (default_rng(5)): H a rank-min(3, Mr, Mt) complex Gaussian product over sqrt(r), Omega with max(1, Mr // 2) ones per
column, OH = Omega .* (H + 0.05 noise), rho in {0.1, 0.5}, tau = c rho sigma_max(OH) with c in {0.02, 0.3} (the second keeps the
threshold active), Imax = 30.  Shapes: the Gram on either side (8 x 12, 12 x 8), the in-LDS Jacobi (32 x 140, 70 x 40), the
global-memory Jacobi (72 x 80, n = 72) and one row (1 x 5).  Bounds: those of jstsp_proposed_algorithm_f64 (include/jstsp.h) -
X within 1e-10 of max|X_ref|, convergence_error within 1e-8; a float64 Gram-route restatement on the CPU differs from the oracle
by at most 4.9e-15 (mc_svt X), 6.1e-14 (mc_admm X) and 2.1e-15 (ce) on these inputs."""
import ctypes as C

import numpy as np
import pytest

from conftest import check_below, ce_rel, load_golden, rel_err
from oracle import solvers as O

pytestmark = pytest.mark.gpu

SHAPES = [(8, 12), (12, 8), (32, 140), (70, 40), (72, 80), (1, 5)]
PARAMS = [(0.1, 0.02), (0.5, 0.3)]
IMAX = 30
TOL_X, TOL_CE = 1e-10, 1e-8
_CASES = {}


def c_(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def case(shape):
    """inputs and the two references per (rho, c), computed once."""
    if shape not in _CASES:
        Mr, Mt = shape
        rng = np.random.default_rng(5)
        r = min(3, Mr, Mt)
        H = c_(rng, Mr, r) @ c_(rng, r, Mt) / np.sqrt(r)
        Omega = np.zeros((Mr, Mt))
        for j in range(Mt):
            Omega[rng.choice(Mr, max(1, Mr // 2), replace=False), j] = 1.0
        OH = Omega * (H + 0.05 * c_(rng, Mr, Mt))
        refs = []
        for rho, c in PARAMS:
            tau = c * rho * np.linalg.norm(OH, 2)
            refs.append(dict(rho=rho, tau=tau, X_svt=O.mc_svt(OH, Omega, IMAX, tau, rho), admm=O.mc_admm(H, OH, Omega, IMAX, tau, rho)))
        _CASES[shape] = dict(H=H, Omega=Omega, OH=OH, refs=refs)
    return _CASES[shape]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_the_oracle(shape):
    import jstsp19_amd as J
    cs = case(shape)
    for ref in cs["refs"]:
        X = J.mc_svt_f64(cs["OH"], cs["Omega"], IMAX, ref["tau"], ref["rho"])
        assert X.dtype == np.complex128
        e = rel_err(X, ref["X_svt"])
        Xa, ce = J.mc_admm_f64(cs["H"], cs["OH"], cs["Omega"], IMAX, ref["tau"], ref["rho"])
        ea, ec = rel_err(Xa, ref["admm"][0]), ce_rel(ce, ref["admm"][1])
        print("%dx%d rho %.1f: mc_svt X %.3g, mc_admm X %.3g ce %.3g, rank(X_svt) %d" %
              (shape + (ref["rho"], e, ea, ec, np.linalg.matrix_rank(ref["X_svt"], tol=1e-9))))
        assert np.abs(ref["X_svt"]).max() > 0 and np.abs(ref["admm"][0]).max() > 0
        check_below("mc64.mc_svt.X", e, TOL_X)
        check_below("mc64.mc_admm.X", ea, TOL_X)
        check_below("mc64.mc_admm.ce", ec, TOL_CE)
        Xn, none = J.mc_admm_f64(None, cs["OH"], cs["Omega"], IMAX, ref["tau"], ref["rho"], want_ce=False)     # ce_out = Htrue = NULL
        assert none is None and same_bits(Xn, Xa)


def test_a_batch_of_three_equals_three_single_calls_and_device_equals_host():
    import torch
    import jstsp19_amd as J
    dev = torch.device("cuda:0")
    for shape in ((12, 8), (70, 40), (72, 80)):
        cs = case(shape)
        rng = np.random.default_rng(6)
        OH = np.stack([cs["OH"], cs["OH"] * 0.5, cs["Omega"] * c_(rng, *shape)])
        H = np.stack([cs["H"], cs["H"] * 0.5, c_(rng, *shape)])
        Om = np.stack([cs["Omega"]] * 3)
        rho = np.array([0.1, 0.5, 0.3])
        tau = np.array([0.02, 0.3, 0.1]) * rho * np.array([np.linalg.norm(OH[t], 2) for t in range(3)])
        Xb = J.mc_svt_f64(OH, Om, IMAX, tau, rho)
        Xab, ceb = J.mc_admm_f64(H, OH, Om, IMAX, tau, rho)
        for t in range(3):
            assert same_bits(Xb[t], J.mc_svt_f64(OH[t], Om[t], IMAX, tau[t], rho[t])), (shape, t)
            Xa, ce = J.mc_admm_f64(H[t], OH[t], Om[t], IMAX, tau[t], rho[t])
            assert same_bits(Xab[t], Xa) and same_bits(ceb[t], ce), (shape, t)
        again = J.mc_svt_f64(OH, Om, IMAX, tau, rho)
        assert same_bits(again, Xb), shape
        t_ = lambda a: J.colmajor(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        Xd = J.mc_svt_f64(t_(OH), t_(Om), IMAX, tau, rho)
        Xad, ced = J.mc_admm_f64(t_(H), t_(OH), t_(Om), IMAX, tau, rho)
        torch.cuda.synchronize()
        assert same_bits(Xd.cpu().numpy(), Xb) and same_bits(Xad.cpu().numpy(), Xab) and same_bits(ced.cpu().numpy(), ceb), shape
        # complex64 / float32 inputs are widened exactly
        X32 = J.mc_svt_f64(OH.astype(np.complex64), Om.astype(np.float32), IMAX, tau, rho)
        assert same_bits(X32, J.mc_svt_f64(OH.astype(np.complex64).astype(np.complex128), Om, IMAX, tau, rho))


def test_imax_zero_returns_zeros_and_order_513_is_refused():
    import jstsp19_amd as J
    cs = case((8, 12))
    X = J.mc_svt_f64(cs["OH"], cs["Omega"], 0, 0.1, 0.1)
    Xa, _ = J.mc_admm_f64(None, cs["OH"], cs["Omega"], 0, 0.1, 0.1, want_ce=False)
    assert X.shape == (8, 12) and not X.any() and not Xa.any()
    lib, ctx = J.load(), J.default_context(0)
    one = (C.c_double * 1)(0.1)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    z, om, x = np.zeros(513 * 513, np.complex128), np.ones(513 * 513), np.zeros(513 * 513, np.complex128)
    assert lib.jstsp_mc_svt_f64(ctx.handle, 513, 513, 1, p(z), p(om), 2, one, one, p(x), 0) == -3          # JSTSP_E_UNSUPPORTED
    assert lib.jstsp_mc_admm_f64(ctx.handle, 513, 513, 1, None, p(z), p(om), 2, one, one, p(x), None, 0) == -3
    assert lib.jstsp_mc_svt_f64(ctx.handle, 512, 513, 1, None, p(om), 2, one, one, p(x), 0) == -1          # JSTSP_E_NULL
    ce = np.zeros(2)
    assert lib.jstsp_mc_admm_f64(ctx.handle, 4, 4, 1, None, p(z), p(om), 2, one, one, p(x), p(ce), 0) == -1  # ce needs Htrue


def test_the_committed_mc_golden():
    import jstsp19_amd as J
    g = load_golden("mc")
    a = (g["OH"], g["Omega"], int(g["Imax"]), float(g["tau"]), float(g["rho"]))
    check_below("mc64.golden.mc_svt.X", rel_err(J.mc_svt_f64(*a), g["X_svt"]), TOL_X)
    X, ce = J.mc_admm_f64(g["Htrue"], *a)
    check_below("mc64.golden.mc_admm.X", rel_err(X, g["X_admm"]), TOL_X)
    check_below("mc64.golden.mc_admm.ce", ce_rel(ce, g["ce_admm"]), TOL_CE)


def test_svt_f64_and_proposed_f64_still_meet_their_goldens():
    """Svt64 moved to csrc/svt64.h: the two entries that used it before must compute what they computed (the existing goldens,
    the existing bounds of tests/test_gpu_f64_proposed.py)."""
    import jstsp19_amd as J
    g = load_golden("svt")
    for i in range(int(g["n"])):
        check_below("mc64.regression.svt_f64", rel_err(J.svt_f64(g["Y%d" % i], float(g["tau%d" % i])), g["X%d" % i]), 1e-10)
    g = load_golden("proposed_small")
    S, Y, ce = J.proposed_algorithm_f64(g["subY"], g["Omega"], g["A"], g["B"], int(g["Imax"]), float(g["tau_Y"]), float(g["tau_Z"]),
                                        float(g["rho"]), "approximate")
    check_below("mc64.regression.proposed_f64.S", rel_err(S, g["S_approximate"]), 1e-10)
    check_below("mc64.regression.proposed_f64.Y", rel_err(Y, g["Y_approximate"]), 1e-10)
    check_below("mc64.regression.proposed_f64.ce", ce_rel(ce, g["ce_approximate"]), 1e-8)
