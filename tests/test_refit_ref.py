"""tests/refit_ref.py, the float64 restatement of the re-fit (jstsp_refit_f64), checked before anything is compared with it:
against the closed form where there is one, on a noiseless problem, as a descent method, as a well-conditioned function of its
input on every problem of tests/test_gpu_refit64.py, and on a tie across the boundary of the support.  No GPU."""
import numpy as np
import pytest

import refit_problems as Q
import refit_ref as F
import resume_problems as P


def _c(rng, *s):
    return rng.standard_normal(s) + 1j * rng.standard_normal(s)


def _conditioned(rng, r, c):
    """r x c with singular values spread over [1, 1.5]: the test is about WHERE the iteration converges, and the Gram of
    kron(B.', A) then has condition <= 1.5^4, so that 60 steps are far more than enough (rate 0.39 per step)."""
    U, _, Vh = np.linalg.svd(_c(rng, r, c), full_matrices=False)
    return (U * np.linspace(1.0, 1.5, min(r, c))) @ Vh


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- (a) Omega all ones, every entry, 60 steps: pinv(A) subY pinv(B) ------------------------------------------------------------
@pytest.mark.parametrize("shapeA,from_zero", [((12, 8), False), ((8, 12), True)])
def test_full_sampling_gives_the_pseudo_inverse_solution(shapeA, from_zero):
    """A 12 x 8 (full column rank: the least-squares solution is unique, any start) and A 8 x 12 (rank-deficient K2: from zero
    conjugate gradients stay in the range of the adjoint and end at the minimum-norm solution), B 6 x 10.  The singular operator
    of the second case needs the stopping rule: with lam = 0 and tol = 0 the steps after convergence divide rounding noise by the
    curvature of null-space directions and diverge (measured: 4e-15 after 30 steps, 1e-2 after 40), which is what tol is for."""
    rng = np.random.default_rng([1, shapeA[0]])
    A, B = _conditioned(rng, *shapeA), _conditioned(rng, 6, 10)
    N, Gr, G2, M = shapeA[0], shapeA[1], 6, 10
    subY = _c(rng, N, M)
    S_in = np.zeros((Gr, G2), complex) if from_zero else _c(rng, Gr, G2)
    x, steps, resid = F.refit(subY, np.ones((N, M)), A, B, S_in, Gr * G2, 60, tol=1e-12 if from_zero else 0.0)
    assert _rel(x, np.linalg.pinv(A) @ subY @ np.linalg.pinv(B)) < 1e-9
    assert (steps < 60) == from_zero
    assert 1 <= steps <= 60 and np.isfinite(resid[:steps + 1]).all() and np.isnan(resid[steps + 1:]).all()


# ---- (b) a noiseless problem whose support lies inside the top K of S_in ----------------------------------------------------------
def test_noiseless_problem_returns_the_sparse_solution():
    rng = np.random.default_rng(2)
    N, M, Gr, G2, K = 16, 20, 8, 6, 10
    A, B = _c(rng, N, Gr) / 4, _c(rng, G2, M) / 2
    flat = np.zeros(Gr * G2, complex)
    sup = rng.choice(Gr * G2, 4, replace=False)
    flat[sup] = 3 * _c(rng, 4)
    S0 = flat.reshape(Gr, G2, order="F")
    Om = (rng.random((N, M)) < 0.5).astype(float)
    S_in = S0 * (1 + 0.3 * _c(rng, Gr, G2)) + 0.05 * _c(rng, Gr, G2)               # wrong values, the right strong entries
    assert set(F.order_of(S_in)[:K] - 1) >= set(sup)
    x, steps, _ = F.refit(Om * (A @ S0 @ B), Om, A, B, S_in, K, 12)
    assert _rel(x, S0) < 1e-10
    assert np.count_nonzero(x) <= K


# ---- (c) the objective does not increase from step to step -------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q.NAMES)
@pytest.mark.parametrize("K", Q.KS)
@pytest.mark.parametrize("lam", Q.LAMS)
def test_objective_does_not_increase(name, K, lam):
    subY, Om, A, B, S_in = Q.trial(name, False, 0)
    tr = []
    F.refit(subY, Om, A, B, S_in, Q.k_of(name, K), 6, lam, trace=tr)
    f = [F.objective(subY, Om, A, B, x, lam) for x in tr]
    assert len(f) == 7
    for a, b in zip(f, f[1:]):
        assert b <= a * (1 + 1e-13)                  # (rounding of the objective itself, 4480 terms)
    assert f[-1] < f[0]


# ---- (d) conditioning: what makes a tolerance on the device result meaningful --------------------------------------------------------
def _perturbed(S_in, rng):
    return S_in * (1 + 1e-15 * rng.standard_normal(S_in.shape))


@pytest.mark.parametrize("name", Q.NAMES)
@pytest.mark.parametrize("shared_B", [False, True])
def test_a_rounding_level_perturbation_of_the_input_moves_the_result_by_rounding(name, shared_B):
    """Every (K, iters, lam, trial) of the GPU test: S_in (1 + 1e-15 n) moves the result by at most 1e-12 of max|S| (measured
    below 1e-13) and no step count."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for t in range(P.BATCH):
        subY, Om, A, B, S_in = Q.trial(name, shared_B, t)
        for K in Q.KS:
            for iters in Q.ITERS:
                for lam in Q.LAMS:
                    k = Q.k_of(name, K)
                    x, n, _ = F.refit(subY, Om, A, B, S_in, k, iters, lam)
                    y, n2, _ = F.refit(subY, Om, A, B, _perturbed(S_in, rng), k, iters, lam)
                    assert n == n2 == iters
                    worst = max(worst, _rel(y, x))
    print("refit_ref conditioning %s shared_B=%s: %.3g" % (name, shared_B, worst))
    assert worst <= 1e-12


def test_the_larger_problem_is_as_well_conditioned():
    b = Q.big()
    args = (b["subY"][0], b["Omega"][0], b["A"], b["B"])
    x, n, _ = F.refit(*args, b["S_in"][0], Q.BIG_K, Q.BIG_ITERS)
    y, n2, _ = F.refit(*args, _perturbed(b["S_in"][0], np.random.default_rng(5)), Q.BIG_K, Q.BIG_ITERS)
    assert n == n2 == Q.BIG_ITERS and _rel(y, x) <= 1e-12


# ---- (e) a tie across the boundary of the support resolves by index ------------------------------------------------------------------
def test_a_tie_across_the_boundary_resolves_by_index():
    rng = np.random.default_rng(6)
    N, M, Gr, G2 = 10, 12, 5, 4
    A, B = _c(rng, N, Gr), _c(rng, G2, M)
    subY, Om = _c(rng, N, M), np.ones((N, M))
    flat = 0.01 * _c(rng, Gr * G2)
    flat[2] = 4.0j
    flat[[11, 6, 14]] = [3 + 4j, 5.0, -4 + 3j]                                  # three entries of equal |z|^2 = 25 (exact)
    flat[17] = 7.0
    S_in = flat.reshape(Gr, G2, order="F")
    # magnitudes: 7 (17), 5 (6, 11, 14 tie), 4 (2): K = 3 takes 17 and the two ties of lowest index, K = 4 all three
    m3, m4 = F.support_mask(S_in, 3), F.support_mask(S_in, 4)
    assert sorted(np.flatnonzero(m3.reshape(-1, order="F"))) == [6, 11, 17]
    assert sorted(np.flatnonzero(m4.reshape(-1, order="F"))) == [6, 11, 14, 17]
    x, _, _ = F.refit(subY, Om, A, B, S_in, 3, 4)
    assert sorted(np.flatnonzero(x.reshape(-1, order="F"))) == [6, 11, 17]
    # and an indx_S overrides the magnitudes: its first K entries, out-of-range ones ignored
    ix = np.array([15, 0, 99, 3, 1], dtype=np.int32)
    m = F.support_mask(S_in, 4, ix)
    assert sorted(np.flatnonzero(m.reshape(-1, order="F"))) == [2, 14]
