"""sparse_admm in float64, jstsp_sparse_admm_f64 (csrc/sparse_admm64.hip), against oracle/solvers.py sparse_admm (the structured
form) and, at 4 x 3, against the line-by-line sparse_admm_literal (dense kron + dense solve).

Shapes: unitary DFT dictionaries at 8 x 8 and 12 x 8 (all Gram eigenvalues equal: the drivers' case, any orthonormal basis is an
eigenbasis); Dr = Q1 diag(d) Q2 with d in [0.5, 2] at 12 x 9 (every lr lt >= 0.0625, well away from rho = 0.01); 72 x 8, whose
Gram of Dr takes the global-memory Jacobi.  Bounds, those of jstsp_mc_admm_f64: S within 1e-10 of max|S_ref|, convergence_error
within 1e-8 relative.  Then: a batch of three returns the bits of the single calls (also at 72), device memory returns the host
bits, ce_out = NULL works with Htrue = NULL, Imax = 0 returns zeros, a NaN in Dr is JSTSP_E_ILLCOND."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import ce_rel, check_below, rel_err
from oracle import solvers as O

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
TOL_S, TOL_CE = 1e-10, 1e-8
IMAX = 12


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _dft(n):
    k = np.arange(n)
    return np.exp(-2j * np.pi * np.outer(k, k) / n) / np.sqrt(n)


def _spread(rng, n):
    q1, _ = np.linalg.qr(_c(rng, n, n))
    q2, _ = np.linalg.qr(_c(rng, n, n))
    return q1 @ np.diag(np.linspace(0.5, 2.0, n)) @ q2


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(Dr, Dt, H (3, Mr, Mt), OH, Imax, S_ref, ce_ref): three trials, the oracle computed once"""
    rng = np.random.default_rng(sum(map(ord, name)))
    Mr, Mt, kind = {"dft8x8": (8, 8, "dft"), "dft12x8": (12, 8, "dft"), "spread12x9": (12, 9, "spread"), "dft72x8": (72, 8, "dft"),
                    "lit4x3": (4, 3, "spread")}[name]
    Dr, Dt = (_dft(Mr), _dft(Mt)) if kind == "dft" else (_spread(rng, Mr), _spread(rng, Mt))
    Imax = 30 if name == "lit4x3" else IMAX
    H, OH = [], []
    for _ in range(3):
        S0 = np.zeros((Mr, Mt), complex)
        sup = rng.choice(Mr * Mt, 4, replace=False)
        S0.reshape(-1)[sup] = _c(rng, 4)
        h = Dr @ S0 @ Dt.conj().T
        H.append(h)
        OH.append((h + 0.05 * _c(rng, Mr, Mt)) * (rng.random((Mr, Mt)) < 0.7))
    ref = [(O.sparse_admm_literal if name == "lit4x3" else O.sparse_admm)(h, oh, Dr, Dt, Imax) for h, oh in zip(H, OH)]
    return dict(Dr=Dr, Dt=Dt, H=np.stack(H), OH=np.stack(OH), Imax=Imax, S_ref=np.stack([r[0] for r in ref]), ce_ref=np.stack([r[1] for r in ref]))


def _cm(a):
    return np.ascontiguousarray(np.swapaxes(np.asarray(a, np.complex128), -1, -2)).reshape(-1)


def solve(Dr, Dt, H, OH, Imax, memspace=HOST, want_ce=True, expect=0):
    """one call through the C ABI on b trials: (S (b, Mr, Mt), ce (b, Imax) or None)"""
    import jstsp19_amd as J
    lib, ctx = J.load(), J.default_context(0)
    b, Mr, Mt = OH.shape
    arrs = [_cm(H) if want_ce else None, _cm(OH), _cm(Dr), _cm(Dt)]
    S = np.full(b * Mr * Mt, np.nan + 1j * np.nan, np.complex128)
    ce = np.full(b * max(Imax, 1), np.nan) if want_ce else None
    if memspace == DEVICE:
        import torch
        ctx.use_torch_stream()
        dev = torch.device("cuda:0")
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
        ta, tS, tce = [up(a) for a in arrs], up(S), up(ce)
        p = lambda t: None if t is None else t.data_ptr()
    else:
        ta, tS, tce = arrs, S, ce
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.jstsp_sparse_admm_f64(ctx.handle, Mr, Mt, Dr.shape[1], Dt.shape[1], b, p(ta[0]), p(ta[1]), p(ta[2]), p(ta[3]), Imax, p(tS), p(tce), memspace)
    assert rc == expect, (rc, lib.jstsp_last_error())
    if rc:
        return None, None
    if memspace == DEVICE:
        import torch
        torch.cuda.synchronize()
        S, ce = tS.cpu().numpy(), None if tce is None else tce.cpu().numpy()
    return np.swapaxes(S.reshape(b, Mt, Mr), 1, 2), None if ce is None or Imax == 0 else ce.reshape(b, Imax)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["dft8x8", "dft12x8", "spread12x9", "dft72x8", "lit4x3"])
def test_against_the_oracle_alone_in_a_batch_and_from_device_memory(name):
    c = case(name)
    if name == "spread12x9":
        lr, lt = np.linalg.eigvalsh(c["Dr"].conj().T @ c["Dr"]), np.linalg.eigvalsh(c["Dt"].conj().T @ c["Dt"])
        assert np.min(np.outer(lr, lt)) >= 0.06                   # every denominator lr lt - rho well away from 0
    S3, ce3 = solve(c["Dr"], c["Dt"], c["H"], c["OH"], c["Imax"])
    for t in range(3):
        S1, ce1 = solve(c["Dr"], c["Dt"], c["H"][t:t + 1], c["OH"][t:t + 1], c["Imax"])
        es, ec = rel_err(S1[0], c["S_ref"][t]), ce_rel(ce1[0], c["ce_ref"][t])
        print("%s trial %d rel_err(S) %.3g  ce %.3g" % (name, t, es, ec))
        check_below("sadmm64.%s.S" % name, es, TOL_S)
        check_below("sadmm64.%s.ce" % name, ec, TOL_CE)
        assert same_bits(S3[t], S1[0]) and same_bits(ce3[t], ce1[0]), (name, t)          # the batch of three: the single calls' bits
    Sd, ced = solve(c["Dr"], c["Dt"], c["H"], c["OH"], c["Imax"], DEVICE)
    assert same_bits(Sd, S3) and same_bits(ced, ce3), name
    Sn, cen = solve(c["Dr"], c["Dt"], None, c["OH"], c["Imax"], HOST, want_ce=False)     # ce_out = NULL, Htrue = NULL
    assert cen is None and same_bits(Sn, S3), name
    Sn, _ = solve(c["Dr"], c["Dt"], None, c["OH"], c["Imax"], DEVICE, want_ce=False)
    assert same_bits(Sn, S3), name
    S2, _ = solve(c["Dr"], c["Dt"], c["H"], c["OH"], c["Imax"])                          # a repeated call
    assert same_bits(S2, S3), name


def test_imax_zero_returns_zeros_and_a_nan_in_dr_is_illcond():
    c = case("dft12x8")
    for mem in (HOST, DEVICE):
        S, ce = solve(c["Dr"], c["Dt"], c["H"], c["OH"], 0, mem)
        assert S.shape == (3, 12, 8) and not np.any(S) and ce is None
    for n, bad in (("dft12x8", np.nan), ("dft72x8", np.nan), ("dft12x8", np.inf)):
        c = case(n)
        Dr = c["Dr"].copy()
        Dr[3, 2] = bad
        solve(Dr, c["Dt"], c["H"], c["OH"], c["Imax"], expect=-6)                        # JSTSP_E_ILLCOND, before the first iteration
    Dt = c["Dt"].copy()
    Dt[1, 1] = np.nan
    solve(c["Dr"], Dt, c["H"], c["OH"], c["Imax"], expect=-6)


def test_the_wrapper_and_the_argument_rules():
    import torch
    import jstsp19_amd as J
    c = case("spread12x9")
    S3, ce3 = solve(c["Dr"], c["Dt"], c["H"], c["OH"], c["Imax"])
    S, ce = J.sparse_admm_f64(c["H"], c["OH"], c["Dr"], c["Dt"], c["Imax"])
    assert S.dtype == np.complex128 and same_bits(S, S3) and same_bits(ce, ce3)
    S, ce = J.sparse_admm_f64(None, c["OH"][0], c["Dr"], c["Dt"], c["Imax"], want_ce=False)
    assert ce is None and same_bits(S, S3[0])
    dev = torch.device("cuda:0")
    t = lambda a: J.colmajor(torch.from_numpy(np.asarray(a, np.complex128)).to(dev))
    St, cet = J.sparse_admm_f64(t(c["H"]), t(c["OH"]), t(c["Dr"]), t(c["Dt"]), c["Imax"])
    torch.cuda.synchronize()
    assert St.is_cuda and same_bits(St.cpu().numpy(), S3) and same_bits(cet.cpu().numpy(), ce3)
    with pytest.raises(J.JstspError) as e:
        J.sparse_admm_f64(np.zeros((1, 513, 4), complex), np.zeros((1, 513, 4), complex), np.eye(513, dtype=complex), np.eye(4, dtype=complex), 2)
    assert e.value.code == -3
    lib, ctx = J.load(), J.default_context(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros(64, np.complex128)
    assert lib.jstsp_sparse_admm_f64(ctx.handle, 4, 3, 5, 3, 1, p(z), p(z), p(z), p(z), 2, p(z), None, HOST) == -2        # Gr != Mr
    assert lib.jstsp_sparse_admm_f64(ctx.handle, 4, 3, 4, 3, 1, None, p(z), p(z), p(z), 2, p(z), p(z.view(np.float64)), HOST) == -1
